"""GPU tier (`-m gpu`) for the search within a doc-id set: Index.search_docs (nxs_index_search_docs_batch,
nxsgpu_search_docs: k_ds_ord / k_ds_score / k_replay).

Truth is docset_truth.py: the unchanged CPU oracle at an unbounded limit, the docs of the set kept in descending doc
id, oracle_lib.topk at the limit.  Everything is compared in full: ids, order, score bits, total, explanations.
Every test takes both routes -- the device pass and NXS_GPU_DOCSET=host -- and the profile's counters prove which one
ran."""
import contextlib
import ctypes as C
import json
import random
import re

import numpy as np
import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from docset_truth import Truth, check_docs, check_explain
from explain_truth import bits

pytestmark = pytest.mark.gpu

ROUTES = pytest.mark.parametrize("route", [None, "host"], ids=["device", "host"])
ALGOS = {"BM25": O.BM25, "TF-IDF": O.TF_IDF}
INVALID, LIMIT = 3, 6
DOCSET_MAX = 1 << 22


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def set_route(monkeypatch, gidx, route, chunk=None, ws=None):
    """NXS_GPU_DOCSET: None = the device pass, "host" = the host lanes; NXS_GPU_DOCSET_CHUNK / _WS"""
    for key, v in (("NXS_GPU_DOCSET", route), ("NXS_GPU_DOCSET_CHUNK", chunk), ("NXS_GPU_DOCSET_WS", ws)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(v))
    gidx.reconfigure()


@contextlib.contextmanager
def routed(monkeypatch, gidx, route, chunk=None, ws=None):
    """the body's queries take `route`, and only that route: the profile's counters say so"""
    set_route(monkeypatch, gidx, route, chunk, ws)
    gidx.search_docs_profile(reset=True)
    try:
        yield
        prof = gidx.search_docs_profile()
        took, other = ("device_cells", "host_cells") if route is None else ("host_cells", "device_cells")
        assert prof[took] > 0 and prof[other] == 0 and prof["passes"] > 0, (route, prof)
    finally:
        set_route(monkeypatch, gidx, None)


def make(path, name, docs, removed=()):
    t, d, _ = nxsfmt.write_index(str(path), name, docs, removed=removed)
    return t, d, Truth(O.Index(t, d), docs, removed)


def check(gidx, truth, qs, docs, S=None, algo="BM25", limit=10, fuzzymatch=False, ctx=None, **kw):
    """one Index.search_docs batch (total on) against the truth; `docs` as the call takes it, S the id set(s) the truth
    keeps (default: `docs` itself, shared); a query the oracle rejects must be rejected with its code"""
    got = gidx.search_docs(qs, docs, limit=limit, algo=algo, fuzzymatch=fuzzymatch, total=True, **kw)
    assert len(got) == len(qs)
    for i, (q, g) in enumerate(zip(qs, got)):
        c = (ctx, i, q[:70], algo, limit)
        Si = docs if S is None else S[i] if isinstance(S, list) else S
        try:
            want = truth.search_docs(q, ALGOS[algo], limit, Si, fuzzymatch)
        except O.SearchError as e:
            assert isinstance(g, N.NxsError) and g.code == e.code, (c, g)
            continue
        check_docs(g, want, c)
    return got


# ---- 1. the tie corpus ---------------------------------------------------------------------------------

TIE_LIMITS = (1, 3, 10, 64, 65, 100)
TIE_SHARES = (0.02, 0.30, 0.80)
VOCAB = ["v%d" % i for i in range(12)]
# 9 doc shapes over the 12 words: few distinct (length, tf) combinations, so scores tie in long runs
SHAPES = [["v0", "v1"], ["v0", "v2"], ["v1", "v2"], ["v0", "v3"], ["v0", "v1", "v4", "v5"], ["v2", "v3", "v6", "v7"],
          ["v0", "v0", "v8", "v9"], ["v1", "v3", "v10", "v11"], ["v4", "v6", "v8", "v10"]]
TIE_QUERIES = ["v0", "v0 OR v1", "v0 OR v1 OR v2 OR v3 OR v4", " OR ".join(VOCAB[:10]), "v0 AND v1", "v0 AND NOT v2",
               "(v0 OR v1) AND (v2 OR v3)", "v0 OR v0 OR v3"]


def tie_docs():
    rng = random.Random(288)
    docs = [(1000 + 7 * i + (1 << 33) * (i % 2), list(rng.choice(SHAPES))) for i in range(700)]
    removed = [docs[i][0] for i in range(36, 700, 37)]
    return docs, removed


@pytest.fixture(scope="module")
def tie(tmp_path_factory):
    """the corpus, its truth, the three sets, and the preconditions asserted from the oracle alone"""
    docs, removed = tie_docs()
    t, d, truth = make(tmp_path_factory.mktemp("tie"), "tie", docs, removed)
    rng = random.Random(37)
    live = truth.live
    assert len(live) == 700 - len(removed) == 682
    sets = []
    for share in TIE_SHARES:
        s = rng.sample(live, int(share * len(live))) + [999, removed[3]]        # one unknown id, one removed id
        rng.shuffle(s)
        sets.append(s)
    cases = [(q, a, k, si) for q in TIE_QUERIES for a in ALGOS for k in TIE_LIMITS for si in range(len(sets))]
    assert len(cases) == 288
    # the truth with S = all live docs is the oracle's search at that limit, in every case
    for q in TIE_QUERIES:
        for a in ALGOS:
            for k in TIE_LIMITS:
                rows, n = truth.search_docs(q, ALGOS[a], k, live)
                plain = truth.oidx.search(q, algo=ALGOS[a], limit=k, fuzzymatch=False)
                assert [(x, bits(s)) for x, s in rows] == [(x, bits(s)) for x, s in plain], (q, a, k)
                assert n == len(truth.all(q, ALGOS[a]))
    # ... and it is none of the three shortcuts in at least half of the cases
    differ = [0, 0, 0]
    for q, a, k, si in cases:
        S = set(sets[si])
        rows = [(x, bits(s)) for x, s in truth.search_docs(q, ALGOS[a], k, S)[0]]
        kept = truth.kept(q, ALGOS[a], S)
        cut = [(x, bits(s)) for x, s in truth.oidx.search(q, algo=ALGOS[a], limit=k, fuzzymatch=False) if x in S]
        by_desc = [(x, bits(s)) for x, s in sorted(kept, key=lambda r: (-r[1], -r[0]))[:k]]
        by_asc = [(x, bits(s)) for x, s in sorted(kept, key=lambda r: (-r[1], r[0]))[:k]]
        for j, other in enumerate((cut, by_desc, by_asc)):
            differ[j] += rows != other
    assert min(differ) >= len(cases) // 2, differ
    return t, d, truth, sets, differ


@ROUTES
@pytest.mark.parametrize("algo", list(ALGOS))
def test_tie_corpus(nxs, tie, monkeypatch, route, algo):
    """8 queries x 6 limits x 3 sets per ranking function: 144 of the 288 cases, both routes"""
    t, d, truth, sets, differ = tie
    gidx = nxs.open_files(t, d)
    try:
        with routed(monkeypatch, gidx, route):
            for k in TIE_LIMITS:
                for si, s in enumerate(sets):
                    check(gidx, truth, TIE_QUERIES, s, algo=algo, limit=k, ctx=("tie", si))
    finally:
        gidx.close()


# ---- 2. boundaries ---------------------------------------------------------------------------------------

@ROUTES
def test_small_sets(nxs, tie, monkeypatch, route):
    """sets of 0, 1, 63, 64 and 65 docs: none, one lane, one round less one, a whole round, a round and a lane"""
    t, d, truth, sets, _ = tie
    gidx = nxs.open_files(t, d)
    hold = [x for x, _ in truth.all("v0 OR v1", O.BM25)]
    qs = ["v0 OR v1", "v0 AND v1", "v2", "nosuchterm"]
    try:
        with routed(monkeypatch, gidx, route):
            for n in (0, 1, 63, 64, 65):
                s = hold[:n]
                for k in (1, 10, 64, 65):
                    got = check(gidx, truth, qs, s, limit=k, ctx=("small", n))
                    assert got[0].total == n and len(got[0]) == min(n, k) and list(got[3]) == [] and got[3].total == 0
            # an empty set as the API has it: n_docs 0 with docs NULL; and through nxs_index_search_docs
            got = gidx.search_docs(["v0"], [None], total=True)
            assert list(got[0]) == [] and got[0].total == 0
            L = N.lib()
            arr = (C.c_uint64 * 3)(hold[5], hold[5], hold[9])             # a duplicate counts once
            r = L.nxs_index_search_docs(gidx._h, None, b"v0 OR v1", 8, arr, 3)
            assert r
            one = N._drain(r)
            L.nxs_resp_release(r)
            check_docs(one, truth.search_docs("v0 OR v1", O.BM25, 1000, {hold[5], hold[9]}), "single", total=False)
            assert len(one) == 2
    finally:
        gidx.close()


def wide_docs(n, seed):
    """n docs that all hold `all`, with a few of 12 frequent words and now and then a rare one: scores tie in runs"""
    rng = random.Random(seed)
    docs = []
    for i in range(n):
        toks = ["all"] + rng.sample(VOCAB, rng.randint(0, 2))
        if i % 97 == 0:
            toks.append("rare%d" % (i % 5))
        docs.append((10 + 3 * i, toks))
    return docs


@pytest.fixture(scope="module")
def six(tmp_path_factory):
    """6 000 docs: two 4096-doc directory words, more than 64 segments at a chunk of 64"""
    return make(tmp_path_factory.mktemp("six"), "six", wide_docs(6000, 6))


@ROUTES
@pytest.mark.parametrize("n", [64 * 64 - 1, 64 * 64, 64 * 64 + 1])
def test_chunk_seams(nxs, six, monkeypatch, route, n):
    """NXS_GPU_DOCSET_CHUNK=64 with sets of 64 x 64 - 1, 64 x 64 and 64 x 64 + 1 matching docs: the replay fetches
    segment counts 64 at a time, so the last set needs a second fetch; the sets straddle doc ordinal 4096"""
    t, d, truth = six
    gidx = nxs.open_files(t, d)
    s = truth.live[900:900 + n]
    qs = ["all", "all OR v1 OR v2", "v3 AND NOT v4", "rare0 OR rare1 OR v5"]
    try:
        with routed(monkeypatch, gidx, route, chunk=64):
            for k in (10, 64, 100, 1000):
                got = check(gidx, truth, qs, s, limit=k, ctx=("seam", n))
                assert got[0].total == n
    finally:
        gidx.close()


@ROUTES
@pytest.mark.parametrize("limit", [1000, 8000, 8001])
def test_large_limits(nxs, six, monkeypatch, route, limit):
    """the heap in LDS at 1000 and 8000, in global memory at 8001; |S| = 5 000 is above the first and below the
    others (capacity min(limit, |S|)), |S| = 300 is below all of them"""
    t, d, truth = six
    gidx = nxs.open_files(t, d)
    qs = ["all", "all OR v1 OR v2 OR v3", "v1 OR v2"]
    try:
        with routed(monkeypatch, gidx, route):
            for n in (5000, 300):
                got = check(gidx, truth, qs, truth.live[500:500 + n], limit=limit, ctx=("limit", n))
                assert len(got[0]) == min(limit, n) and got[0].total == n
    finally:
        gidx.close()


@pytest.fixture(scope="module")
def nine(tmp_path_factory):
    """9 000 docs: a set above 8 001, so the heap in global memory fills up and evicts"""
    return make(tmp_path_factory.mktemp("nine"), "nine", wide_docs(9000, 9))


@ROUTES
def test_global_heap_evicts(nxs, nine, monkeypatch, route):
    t, d, truth = nine
    gidx = nxs.open_files(t, d)
    try:
        with routed(monkeypatch, gidx, route):
            got = check(gidx, truth, ["all OR v1 OR v2", "all"], truth.live, limit=8001, ctx="global")
            assert len(got[0]) == 8001 and got[0].total == 9000
            check(gidx, truth, ["all OR v1 OR v2"], truth.live, limit=8000, ctx="lds full")
    finally:
        gidx.close()


@ROUTES
def test_passes(nxs, six, monkeypatch, route):
    """NXS_GPU_DOCSET_WS too small for two queries: a pass per query that reaches the device, and still every distinct
    set resolved once"""
    t, d, truth = six
    gidx = nxs.open_files(t, d)
    a, b = truth.live[:700], truth.live[300:1500]
    qs = ["all", "v1 OR v2", "nosuchterm", "v3 AND v4", "all AND NOT v1"]
    try:
        with routed(monkeypatch, gidx, route, ws=1):
            got = check(gidx, truth, qs, [a, b, a, a, b], S=[a, b, a, a, b], limit=10, ctx="passes")
            prof = gidx.search_docs_profile()
            assert prof["passes"] == 4 and prof["sets"] == 2 and prof["calls"] == 1, prof
            assert prof["ids"] == len(a) + len(b), prof
            assert prof["candidates"] == sum(g.total for g in got), prof
        with routed(monkeypatch, gidx, route):
            check(gidx, truth, qs, [a, b, a, a, b], S=[a, b, a, a, b], limit=10, ctx="one pass")
            prof = gidx.search_docs_profile()
            assert prof["passes"] == 1 and prof["sets"] == 2 and prof["ids"] == len(a) + len(b), prof
    finally:
        gidx.close()


# ---- 3. lookup paths -------------------------------------------------------------------------------------

def dense_docs():
    """5 000 docs: `all` everywhere (a bitmap row under NXS_GPU_BM_SHARE=1), `dense` in every third doc with an
    outlier tf of 300 in one of them (TF-IDF: beyond the cap), 40 words w0 .. w39 of df ~ 250"""
    rng = random.Random(5)
    docs = []
    for i in range(5000):
        toks = ["all"] + rng.sample(["w%d" % j for j in range(40)], 2)
        if i % 3 == 0:
            toks += ["dense"] * (300 if i == 2400 else rng.randint(1, 3))
        docs.append((5 + 2 * i, toks))
    return docs


@pytest.fixture(scope="module")
def dense(tmp_path_factory):
    return make(tmp_path_factory.mktemp("dense"), "dense", dense_docs())


@ROUTES
@pytest.mark.parametrize("env", [{"NXS_GPU_BM_SHARE": "1"}, {"NXS_GPU_NOBLKMAP": "1"}, {}], ids=["share1", "nomap", "default"])
def test_lookup_paths(nxs, dense, monkeypatch, route, env):
    """terms with and without a block-presence bitmap in one query, a TF-IDF dense term with an outlier tf, queries
    of 9 and 32 tokens (the postfix program)"""
    t, d, truth = dense
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    gidx = nxs.open_files(t, d)
    ws = ["w%d" % j for j in range(40)]
    qs = ["all", "dense", "all AND dense", "dense OR w1", "all AND NOT dense", "(w1 OR w2) AND all",
          " OR ".join(ws[:9]), "(" + " OR ".join(ws[:8]) + ") AND NOT dense", " OR ".join(ws[:32]),
          "(" + " OR ".join(ws[:30]) + ") AND all AND NOT dense"]
    rng = random.Random(3)
    s = rng.sample(truth.live, 1500) + [5 + 2 * 2400]
    try:
        rows = len(gidx.device_image()["bm_terms"])
        if env.get("NXS_GPU_BM_SHARE") == "1":
            assert 1 <= rows < 10, rows                                  # `all` has a row, the w-words have none
        elif "NXS_GPU_NOBLKMAP" in env:
            assert rows == 0
        else:
            assert rows >= 42, rows                                      # every term of the queries has one
        with routed(monkeypatch, gidx, route):
            for algo in ALGOS:
                for k in (10, 100):
                    got = check(gidx, truth, qs, s, algo=algo, limit=k, ctx=("paths", tuple(env)))
            # the regular posting's uncapped float: tf 300, the term's largest impact by far
            got = check(gidx, truth, ["dense"], s, algo="TF-IDF", limit=5000, ctx="outlier")
            w = truth.ex.contrib(b"dense", O.TF_IDF)
            assert got[0][0] == (5 + 2 * 2400, max(w.values())) and got[0][0][1] > 2 * sorted(w.values())[-2]
    finally:
        gidx.close()


# ---- 4. batches ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def words_corpus(tmp_path_factory):
    rng = random.Random(5)
    words = ["linux", "lint", "unix", "erlang", "python", "kernel", "shell", "driver", "thread", "lynx"]
    docs = [(7 * i + 1, rng.sample(words, 3)) for i in range(400)]
    t, d, _ = nxsfmt.write_index(str(tmp_path_factory.mktemp("words")), "words", docs)
    term_ids = {w.encode(): O.Index(t, d).lookup(w.encode()) for w in words}
    return t, d, Truth(O.Index(t, d), docs), words, term_ids


@ROUTES
def test_batches(nxs, words_corpus, monkeypatch, route):
    """per-query sets, one shared set (resolved once, by the counter), identical (query, set) pairs, an empty set; a
    parse error, a 33-term query and an oversized set as errs[i] while the rest is answered"""
    t, d, truth, words, _ = words_corpus
    gidx = nxs.open_files(t, d)
    rng = random.Random(44)
    live = truth.live
    with pytest.raises(O.SearchError) as oe:
        truth.all("broken AND", O.BM25)
    bad_code = oe.value.code
    try:
        with routed(monkeypatch, gidx, route):
            # one shared set: sorted and resolved once
            shared = rng.sample(live, 150)
            qs = ["linux", "linux OR unix", "kernel AND NOT shell", "python AND erlang", "lynx OR lint OR thread"]
            check(gidx, truth, qs, shared, limit=7, ctx="shared")
            prof = gidx.search_docs_profile(reset=True)
            assert prof["sets"] == 1 and prof["ids"] == 150 and prof["passes"] == 1, prof
            assert prof["device_cells" if route is None else "host_cells"] == 5 * 150, prof
            # per-query sets, two entries that are one object, identical (query, set) pairs, an empty set
            sets = [rng.sample(live, rng.randint(1, 200)) for _ in qs]
            sets[3] = sets[1]
            sets[4] = []
            qs2 = qs[:3] + [qs[1], qs[4]]
            got = check(gidx, truth, qs2, sets, S=sets, limit=7, ctx="per query")
            assert got[3] == got[1] and got[3].total == got[1].total and list(got[4]) == [] and got[4].total == 0
            prof = gidx.search_docs_profile(reset=True)
            assert prof["sets"] == 3, prof
            assert gidx.search_docs([], []) == []
            with pytest.raises(N.NxsError) as e:
                gidx.search_docs(["unix"], shared, limit=0)
            assert e.value.code == INVALID
            gidx.search_docs(["unix"], shared)
    finally:
        gidx.close()


@ROUTES
def test_errors_in_a_batch(nxs, tmp_path, monkeypatch, route):
    """a parse error, a query of 33 live terms and an oversized set are errs[i] with the promised codes and messages,
    and the rest of the batch is answered"""
    rng = random.Random(33)
    rare = ["r%d" % i for i in range(40)]
    docs = [(3 * i + 1, rng.sample(rare, 4)) for i in range(200)]
    t, d, truth = make(tmp_path, "rare", docs)
    gidx = nxs.open_files(t, d)
    with pytest.raises(O.SearchError) as oe:
        truth.all("broken AND", O.BM25)
    huge = np.arange(DOCSET_MAX + 1, dtype=np.uint64)
    try:
        with routed(monkeypatch, gidx, route):
            s = truth.live[::2]
            q32, q33 = " OR ".join(rare[:32]), " OR ".join(rare[:33])
            qs = ["r1 OR r2", "broken AND", q33, "r3", q32, "r4 AND NOT r5"]
            got = gidx.search_docs(qs, [s, s, s, huge, s, s], limit=10, total=True, fuzzymatch=False)
            assert isinstance(got[1], N.NxsError) and got[1].code == oe.value.code, got[1]
            assert isinstance(got[2], N.NxsError) and got[2].code == LIMIT, got[2]
            assert isinstance(got[3], N.NxsError) and got[3].code == LIMIT, got[3]
            for i in (0, 4, 5):
                check_docs(got[i], truth.search_docs(qs[i], O.BM25, 10, s), ("errs", i))
            assert len(got[4]) == 10 and got[4].total == len(s)
            # the messages, through the single call
            L = N.lib()
            ids = (C.c_uint64 * len(s))(*s)
            assert not L.nxs_index_search_docs(gidx._h, None, q33.encode(), len(q33), ids, len(s))
            assert gidx.nxs.error() == (LIMIT, "search_docs is not available for a query of more than 32 terms")
            assert not L.nxs_index_search_docs(gidx._h, None, b"r3", 2, huge.ctypes.data_as(C.POINTER(C.c_uint64)), len(huge))
            assert gidx.nxs.error() == (LIMIT, "doc set too large")
            assert not L.nxs_index_search_docs(gidx._h, None, b"broken AND", 10, ids, len(s))
            assert gidx.nxs.error()[0] == oe.value.code
            # exactly 2^22 ids are served
            got = gidx.search_docs(["r3"], huge[:DOCSET_MAX], limit=10, total=True, fuzzymatch=False)
            check_docs(got[0], truth.search_docs("r3", O.BM25, 10, truth.live), "2^22")
    finally:
        gidx.close()


@ROUTES
def test_leaves_total_explain_json(nxs, words_corpus, monkeypatch, route):
    """fuzzy, prefix and wildcard leaves; total and explain together; the JSON"""
    t, d, truth, words, term_ids = words_corpus
    gidx = nxs.open_files(t, d)
    rng = random.Random(45)
    s = rng.sample(truth.live, 220)
    S = set(s)
    df = lambda w: len(truth.ex.tf[w.encode()])
    by_df = lambda ts: sorted(ts, key=lambda w: (-df(w), term_ids[w.encode()]))
    try:
        with routed(monkeypatch, gidx, route):
            # a token that misses the dictionary resolves through the BK walk, exactly as a search's
            check(gidx, truth, ["linus", "linus AND kernel", "pythom OR shel"], s, limit=9, fuzzymatch=True, ctx="fuzzy")
            assert gidx.search_docs(["linus"], s, fuzzymatch=False, total=True)[0].total == 0
            for q, kw, exp in (("lin*", {"prefixmatch": True}, by_df([w for w in words if w.startswith("lin")])),
                               ("l*x AND NOT shell", {"wildcardmatch": True}, by_df([w for w in words if re.fullmatch("l.*x", w)])),
                               ("l?n* OR kernel", {"wildcardmatch": True}, by_df([w for w in words if re.fullmatch("l.n.*", w)]))):
                rw = q.replace(q.split()[0], "(" + " OR ".join(exp) + ")", 1)
                assert len(exp) >= 2
                for k in (3, 50):
                    g = gidx.search_docs([q], s, limit=k, total=True, fuzzymatch=False, **kw)[0]
                    check_docs(g, truth.search_docs(q, O.BM25, k, S, rewritten=rw), (q, k))
            # total and explain together
            qs = ["linux OR unix", "kernel AND NOT shell", "python", "lynx OR lint OR thread OR driver", "nosuchterm"]
            for algo in ALGOS:
                plain = gidx.search_docs(qs, s, limit=12, algo=algo, fuzzymatch=False)
                got = gidx.search_docs(qs, s, limit=12, algo=algo, fuzzymatch=False, total=True, explain=True)
                cells = 0
                for q, g, p in zip(qs, got, plain):
                    check_docs(g, truth.search_docs(q, ALGOS[algo], 12, S), ("explain", q, algo))
                    cells += check_explain(g, p, truth, q, ALGOS[algo], False, ("explain", algo))
                assert cells > 40
            # the JSON is a search's: results, the total, the tokens
            want, n = truth.search_docs("linux OR unix", O.BM25, 3, S)
            js = json.loads(gidx.search_docs(["linux OR unix"], s, limit=3, total=True, fuzzymatch=False, json=True)[0])
            assert [r["doc_id"] for r in js["results"]] == [x for x, _ in want] and js["total"] == n
            assert js == json.loads(O.results_json(want)) | {"total": n}
            js = json.loads(gidx.search_docs(["linux OR unix"], s, limit=3, explain=True, fuzzymatch=False, json=True)[0])
            assert js["tokens"] == ["unix", "linux"] and all("terms" in r for r in js["results"])
    finally:
        gidx.close()


# ---- 5. refresh --------------------------------------------------------------------------------------------

@ROUTES
def test_refresh(nxs, tmp_path, monkeypatch, route):
    """after an in-place append and a removal the same set selects the appended doc and no longer the removed one"""
    ev = [("add", 10, ["apple", "maple", "zebra"]), ("add", 20, ["apple", "apply", "pear"]),
          ("add", 30, ["ample", "apple", "pear"]), ("add", 40, ["apply", "zebra"]), ("add", 50, ["ample", "fig"]),
          ("add", 60, ["apricot", "fig"]), ("add", 70, ["kiwi", "apple"]), ("add", 80, ["lime", "kiwi"]),
          ("add", 90, ["plum", "sloe"]), ("add", 100, ["plum", "lime"]), ("rm", 60)]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 262144)
    open(d, "wb").write(dimg + b"\0" * 262144)
    gidx = nxs.open_files(t, d)
    qs = ["apple", "apple OR fig", "pear AND apple", "apple AND NOT pear", "plum OR kiwi", "quince OR zebra"]
    s = [130, 20, 10, 70, 60, 90, 30, 100, 20, 555]                       # 130 is not there yet, 60 is gone, 555 never comes

    def publish(first=False):
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        if not first:
            nxsfmt.publish_in_place(t, d, timg, dimg)
        return Truth(O.Index(t, d), [(e[1], e[2]) for e in ev if e[0] == "add"], [e[1] for e in ev if e[0] == "rm"])
    try:
        with routed(monkeypatch, gidx, route):
            got = check(gidx, publish(first=True), qs, s, limit=4, ctx="snapshot 0")
            assert [x for x, _ in got[0]] and {x for x, _ in got[0]} <= {10, 20, 30, 70} and got[0].total == 4
            ev.append(("rm", 20))
            ev.append(("add", 130, ["apple", "quince", "zebra", "quince"]))
            got = check(gidx, publish(), qs, s, limit=4, ctx="refreshed")
            ids = {x for x, _ in got[0]}
            assert 130 in ids and 20 not in ids and got[0].total == 4 and [x for x, _ in got[5]] and got[5].total == 2
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 6. in flight, 7. refusals -------------------------------------------------------------------------------

@ROUTES
def test_between_begin_and_end(nxs, words_corpus, monkeypatch, route):
    """a call between _begin and _end of pipelined batches, a fuzzy batch among them: the batches' responses equal a
    plain run bit for bit, the call's equal the truth"""
    t, d, truth, words, _ = words_corpus
    gidx = nxs.open_files(t, d)
    b1 = ["linux OR unix", "kernel AND shell", "python", "driver AND NOT thread"]
    b2 = ["linus OR unix", "pythom", "lynx OR shel"]                      # tokens that miss the dictionary: a fuzzy pass
    mine = ["linux AND unix", "python", "lint OR lynx OR erlang", "kernl OR shell"]
    s = truth.live[::3]
    as_bits = lambda rs: [[(x, bits(v)) for x, v in r] for r in rs]
    try:
        with routed(monkeypatch, gidx, route):
            plain1 = gidx.search_batch(b1, limit=10, fuzzymatch=False, total=True)
            plain2 = gidx.search_batch(b2, limit=10, fuzzymatch=True)
            gidx.search_batch_begin(b1, limit=10, fuzzymatch=False, total=True)
            gidx.search_batch_begin(b2, limit=10, fuzzymatch=True)
            check(gidx, truth, mine, s, limit=8, fuzzymatch=True, ctx="in flight")
            r1 = gidx.search_batch_end()
            assert as_bits(r1) == as_bits(plain1) and [x.total for x in r1] == [x.total for x in plain1]
            assert as_bits(gidx.search_batch_end()) == as_bits(plain2)
    finally:
        gidx.close()


@ROUTES
def test_refusals_and_emulated_world(nxs, words_corpus, monkeypatch, route):
    from nxsearch_amd import multi as M
    t, d, truth, words, _ = words_corpus
    sh = nxs.open_shard(t, d, 0, 1)
    set_route(monkeypatch, sh, route)
    with pytest.raises(N.NxsError) as e:
        sh.search_docs(["linux"], truth.live[:10])
    assert e.value.code == INVALID and e.value.msg == "search_docs is not available on a doc shard"
    set_route(monkeypatch, sh, None)
    sh.close()
    # an emulated world of 2: the call is local -- no collective, the whole batch answered here, total served
    gidx = nxs.open_files(t, d)
    try:
        with routed(monkeypatch, gidx, route):
            M.emulate(gidx, 1, 2)
            check(gidx, truth, ["linux OR unix", "kernel", "python AND NOT shell"], truth.live[::2], limit=6, ctx="world 2")
            M.emulate(gidx, 0, 0)
    finally:
        gidx.close()


def test_an_index_that_is_never_asked_runs_no_pass(nxs, words_corpus):
    t, d, truth, words, _ = words_corpus
    gidx = nxs.open_files(t, d)
    gidx.search_batch(["linux OR unix", "python"], limit=10, total=True, explain=True)
    gidx.related(["linux"])
    zero = {"calls": 0, "passes": 0, "sets": 0, "ids": 0, "device_cells": 0, "host_cells": 0, "candidates": 0, "ord_ms": 0.0,
            "score_ms": 0.0, "replay_ms": 0.0}
    assert gidx.search_docs_profile() == zero
    gidx.search_docs(["nosuchterm", "linux"], [truth.live[:5], None], fuzzymatch=False)       # nothing to score: no pass either
    assert gidx.search_docs_profile() == zero
    gidx.set_profiling(True)
    got = gidx.search_docs(["linux", "linux OR unix"], truth.live[:300], limit=5, total=True, fuzzymatch=False)
    prof = gidx.search_docs_profile(reset=True)
    assert prof["calls"] == 1 and prof["passes"] == 1 and prof["sets"] == 1 and prof["ids"] == 300, prof
    assert prof["device_cells"] == 600 and prof["candidates"] == got[0].total + got[1].total, prof
    assert prof["ord_ms"] > 0 and prof["score_ms"] > 0 and prof["replay_ms"] > 0, prof
    assert gidx.search_docs_profile() == zero
    gidx.close()
