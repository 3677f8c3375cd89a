"""GPU tier (`-m gpu`) for a query's matches listed by doc id: Index.match_docs (nxs_index_match_docs_batch,
nxsgpu_match_docs: k_md_mask / k_md_from / k_md_count / k_md_scan / k_md_emit).

Truth is matchdocs_truth.py: the doc set from the CPU oracle with the limit lifted, sorted ascending, cut at the
cursor and the limit.  Ids, count, total and next are compared in full.  Every test takes both routes -- the device
pass and NXS_GPU_MATCHDOCS=host -- and the profile's counters prove which one ran."""
import contextlib
import ctypes as C
import json
import random
import re

import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
import docset_truth
from matchdocs_truth import Truth, check_page, page_of

pytestmark = pytest.mark.gpu

ROUTES = pytest.mark.parametrize("route", [None, "host"], ids=["device", "host"])
ALGOS = {"BM25": O.BM25, "TF-IDF": O.TF_IDF}
INVALID, LIMIT = 3, 6
MATCH_MAX = 1 << 22
RUN = 64            # NXS_GPU_MATCHDOCS_RUN at its smallest legal value: one wavefront's worth
VOCAB = ["v%d" % i for i in range(12)]


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def set_route(monkeypatch, gidx, route, run=None, ws=None):
    """NXS_GPU_MATCHDOCS: None = the device pass, "host" = the host loop; NXS_GPU_MATCHDOCS_RUN / _WS"""
    for key, v in (("NXS_GPU_MATCHDOCS", route), ("NXS_GPU_MATCHDOCS_RUN", run), ("NXS_GPU_MATCHDOCS_WS", ws)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(v))
    gidx.reconfigure()


@contextlib.contextmanager
def routed(monkeypatch, gidx, route, run=None, ws=None):
    """the body's queries take `route`, and only that route: the profile's counters say so"""
    set_route(monkeypatch, gidx, route, run, ws)
    gidx.match_docs_profile(reset=True)
    try:
        yield
        prof = gidx.match_docs_profile()
        took, other = ("device_pairs", "host_pairs") if route is None else ("host_pairs", "device_pairs")
        assert prof[took] > 0 and prof[other] == 0, (route, prof)
        assert (prof["passes"] > 0) == (route is None), (route, prof)
    finally:
        set_route(monkeypatch, gidx, None)


def make(path, name, docs, removed=()):
    t, d, _ = nxsfmt.write_index(str(path), name, docs, removed=removed)
    return t, d, Truth(O.Index(t, d), docs, removed)


def check(gidx, truth, qs, algo="BM25", limit=None, start=None, fuzzymatch=False, ctx=None):
    """one Index.match_docs batch against the truth; a query the oracle rejects must be rejected with its code"""
    got = gidx.match_docs(qs, limit=limit, start=start, algo=algo, fuzzymatch=fuzzymatch)
    assert len(got) == len(qs)
    for i, (q, g) in enumerate(zip(qs, got)):
        s = 0 if start is None else start[i] if hasattr(start, "__len__") else start
        c = (ctx, q[:70], algo, limit, s)
        try:
            want = truth.page(q, ALGOS[algo], 1000 if limit is None else limit, s, fuzzymatch)
        except O.SearchError as e:
            assert isinstance(g, N.NxsError) and g.code == e.code, (c, g)
            continue
        check_page(g, want, c)
    return got


# ---- 1. run seams, 2. mask tile seams ---------------------------------------------------------------------

def tile_widths():
    w = (C.c_uint32 * 2)()
    L = N.lib()
    L.nxs_test_count_tile_widths.argtypes = [C.POINTER(C.c_uint32)]
    L.nxs_test_count_tile_widths(w)
    return int(w[0]), int(w[1])


@pytest.fixture(scope="module")
def seam_corpora(tmp_path_factory):
    """n docs of two or three tokens around a seam at ordinal E: `all` in every doc, `last` only in the last doc
    before the seam, `first` only in the first doc behind it, `tail` only in the last doc; built once per (E, n),
    shared by the routes"""
    made = {}

    def get(E, n):
        if (E, n) not in made:
            rng = random.Random(n + E)
            docs, did = [], 0
            for i in range(n):
                did += rng.randint(1, 1000)
                toks = [rng.choice(VOCAB) for _ in range(rng.randint(1, 2))] + ["all"]
                if i == E - 1:
                    toks.append("last")
                if i == E:
                    toks.append("first")
                if i == n - 1:
                    toks.append("tail")
                docs.append((did, toks))
            made[(E, n)] = make(tmp_path_factory.mktemp("seam%d_%d" % (E, n)), "seam", docs)
        return made[(E, n)]
    return get


SEAM_QUERIES = ["all", "last", "first", "tail", "v3", "v1 AND v2", "v1 OR last", "all AND NOT last", "all AND NOT first",
                "first OR tail", "last AND first", "v0 AND NOT all", "nosuchterm", "tail AND NOT v1",
                " OR ".join(VOCAB[:8]), "(" + " OR ".join(VOCAB[:7]) + ") AND NOT last",
                " OR ".join(VOCAB[:9]), "(" + " OR ".join(VOCAB[:9]) + ") AND NOT first",
                " OR ".join(VOCAB) + " OR last OR first",
                "(" + " OR ".join(VOCAB[:10]) + ") AND (last OR first OR tail)", " OR ".join(VOCAB) + " OR all"]


@ROUTES
@pytest.mark.parametrize("n", [63, 64, 65, 129, 64 * 256 - 1, 64 * 256, 64 * 256 + 1])
def test_run_seams(nxs, seam_corpora, monkeypatch, route, n):
    """RUN = 64: corpora that end just before, on and just behind a run boundary, and whose number of runs ends just
    before, on and just behind the scan's chunk of 256 runs; queries of 1, 2, 8 and 9 tokens (the last take the
    postfix program), AND / OR / AND NOT, matching every doc, no doc, only the first or last doc of a run and the
    last doc overall; limits at the wavefront's width, cursors at the seam"""
    t, d, truth = seam_corpora(RUN, n)
    gidx = nxs.open_files(t, d)
    live = truth.live
    try:
        with routed(monkeypatch, gidx, route, run=RUN):
            got = check(gidx, truth, SEAM_QUERIES, limit=MATCH_MAX, ctx=("all of it", n))
            assert list(got[0]) == live and got[0].total == n and got[0].next is None
            assert list(got[1]) == ([live[RUN - 1]] if n >= RUN else []) and list(got[2]) == ([live[RUN]] if n > RUN else [])
            assert list(got[3]) == [live[-1]] and list(got[12]) == [] and got[12].total == 0 and got[10].total == 0
            totals = gidx.search_batch(SEAM_QUERIES, limit=1, fuzzymatch=False, total=True)
            assert [g.total for g in got] == [x.total for x in totals]
            for limit in (1, 63, 64, 65):
                check(gidx, truth, SEAM_QUERIES, limit=limit, ctx=("from 0", n))
            # cursors on the last doc of a run, on the first of the next, behind the last doc of the last full run
            for at in sorted({min(RUN - 1, n - 1), min(RUN, n - 1), n - 1 - (n - 1) % RUN, n - 1}):
                check(gidx, truth, SEAM_QUERIES, limit=65, start=live[at], ctx=("from ordinal", at, n))
                check(gidx, truth, SEAM_QUERIES, limit=3, start=live[at] + 1, ctx=("behind ordinal", at, n))
            if n > 64 * 255:
                mid = live[64 * 255 - 2]
                check(gidx, truth, SEAM_QUERIES, limit=130, start=mid, ctx=("the last chunk of runs", n))
    finally:
        gidx.close()


@ROUTES
@pytest.mark.parametrize("which", [0, 1], ids=["u8", "u32"])
def test_mask_tile_seams(nxs, seam_corpora, monkeypatch, route, which):
    """the W + 1 corpus of both widths of the mask tile, with pages that cross the seam; default run"""
    W = tile_widths()[which]
    assert W == (16384, 4096)[which]
    t, d, truth = seam_corpora(W, W + 1)
    gidx = nxs.open_files(t, d)
    live = truth.live
    try:
        with routed(monkeypatch, gidx, route):
            got = check(gidx, truth, SEAM_QUERIES, limit=7, start=live[W - 3], ctx=("across", W))
            assert list(got[0]) == live[W - 3:] and got[0].total == W + 1 and got[0].next is None
            assert list(got[-1]) == live[W - 3:] and list(got[1]) == [live[W - 1]] and list(got[2]) == [live[W]]
            check(gidx, truth, SEAM_QUERIES, limit=2, start=live[W - 2] + 1, ctx=("lands on the seam", W))
            got = check(gidx, truth, SEAM_QUERIES, limit=MATCH_MAX, ctx=("all of it", W))
            assert list(got[0]) == live and list(got[-1]) == live
    finally:
        gidx.close()


# ---- 3. ranking functions, limits, walks, cursors ---------------------------------------------------------

@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """300 docs of one to three words, every seventh removed"""
    rng = random.Random(300)
    docs = [(10 + 3 * i, [rng.choice(VOCAB) for _ in range(rng.randint(1, 3))]) for i in range(300)]
    removed = [d for d, _ in docs[5::7]]
    return make(tmp_path_factory.mktemp("small"), "small", docs, removed)


def random_query(rng, nmax):
    q = rng.choice(VOCAB)
    for _ in range(rng.randint(1, nmax) - 1):
        q += rng.choice([" AND ", " OR ", " AND NOT ", " "]) + rng.choice(VOCAB)
    return q


@ROUTES
@pytest.mark.parametrize("algo", list(ALGOS))
def test_ranking_functions_limits_and_removed_docs(nxs, small, monkeypatch, route, algo):
    t, d, truth = small
    gidx = nxs.open_files(t, d)
    rng = random.Random(17)
    qs = ["v0", "v1 OR v2", "v3 AND v4", "v5 AND NOT v6", " OR ".join(VOCAB)] + [random_query(rng, 11) for _ in range(20)]
    gone = set(x for x in range(10, 910, 3)) - set(truth.live)
    try:
        with routed(monkeypatch, gidx, route):
            m = len(truth.M(qs[4], ALGOS[algo]))
            assert m == len(truth.live)                        # every live doc holds a word of the vocabulary
            for limit in (1, 63, 64, 65, m - 1, m, m + 1, MATCH_MAX, None):
                got = check(gidx, truth, qs, algo=algo, limit=limit, ctx="limits")
            assert all(not (set(g) & gone) for g in got) and list(got[4]) == truth.live
    finally:
        gidx.close()


@ROUTES
def test_ranking_function_that_scores_nothing(nxs, tmp_path, monkeypatch, route):
    """a header with fewer tokens than docs (adl < 1): BM25 scores nothing -- an empty page, total 0; TF-IDF lists"""
    rng = random.Random(5)
    words = ["a%d" % i for i in range(9)]
    docs = [(3 * i + 1, [rng.choice(words) for _ in range(rng.randint(1, 3))]) for i in range(300)]
    timg, _, term_ids = nxsfmt.build_images(docs)
    blocks = []
    for did, toks in docs:
        cnt = {}
        for w in toks:
            cnt[term_ids[w.encode()]] = cnt.get(term_ids[w.encode()], 0) + 1
        blocks.append((did, len(toks), sorted(cnt.items())))
    tp, dp = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(tp, "wb").write(timg)
    open(dp, "wb").write(nxsfmt.dtmap_image(blocks, len(docs) - 1, len(docs)))
    gidx, tr = nxs.open_files(tp, dp), Truth(O.Index(tp, dp), docs)
    qs = ["a0", "a0 OR a1", "a1 AND NOT a2"]
    try:
        with routed(monkeypatch, gidx, route):
            got = check(gidx, tr, qs, algo="BM25", limit=8, ctx="adl < 1")
            assert [(list(g), g.total, g.next) for g in got] == [([], 0, None)] * 3
            got = check(gidx, tr, qs, algo="TF-IDF", limit=8, ctx="tf-idf")
            assert all(len(g) == 8 and g.total > 8 and g.next for g in got)
    finally:
        gidx.close()


@ROUTES
@pytest.mark.parametrize("run", [RUN, None], ids=["run64", "default-run"])
def test_walk(nxs, small, monkeypatch, route, run):
    """pages of 7 from 0 until next is None: concatenated they are M, with the same total on every page"""
    t, d, truth = small
    gidx = nxs.open_files(t, d)
    qs = ["v0 OR v1 OR v2", "v3", "v4 AND NOT v5", " OR ".join(VOCAB[:9])]
    try:
        with routed(monkeypatch, gidx, route, run=run):
            walked, cursors, pages = [[] for _ in qs], [0] * len(qs), 0
            live = list(range(len(qs)))
            while live:
                got = gidx.match_docs([qs[i] for i in live], limit=7, start=[cursors[i] for i in live], fuzzymatch=False)
                pages += 1
                nxt = []
                for i, g in zip(live, got):
                    M = truth.M(qs[i])
                    check_page(g, page_of(M, 7, cursors[i]), ("walk", qs[i], cursors[i]))
                    walked[i] += list(g)
                    if g.next is not None:
                        assert g.next > cursors[i]
                        cursors[i] = g.next
                        nxt.append(i)
                live = nxt
            assert pages == max(-(-len(truth.M(q)) // 7) for q in qs)
            for q, w in zip(qs, walked):
                assert w == truth.M(q) and len(w) > 20, q
    finally:
        gidx.close()


@ROUTES
def test_cursors(nxs, small, monkeypatch, route):
    """the cursor on a match, on a live non-match, on a removed doc, between ids, above the last id, at UINT64_MAX;
    per-query cursors against the params' match_from"""
    t, d, truth = small
    gidx = nxs.open_files(t, d)
    q = "v0 OR v1"
    M = truth.M(q)
    removed = sorted(set(range(10, 910, 3)) - set(truth.live))
    non_match = [x for x in truth.live if x not in set(M)]
    starts = [M[5], M[-1], non_match[3], removed[2], removed[-1], M[7] + 1, M[7] - 1, truth.live[-1] + 1, (1 << 64) - 1, 0, 1]
    assert (M[7] + 1) % 3 != 1                                   # between ids: no doc has this id
    try:
        with routed(monkeypatch, gidx, route):
            per_query = check(gidx, truth, [q] * len(starts), limit=9, start=starts, ctx="per query")
            assert per_query[0][0] == M[5] and list(per_query[1]) == [M[-1]] and list(per_query[7]) == [] and list(per_query[8]) == []
            assert per_query[7].total == len(M) and per_query[8].total == len(M) and per_query[8].next is None
            for s, g in zip(starts, per_query):
                one = check(gidx, truth, [q, "v2"], limit=9, start=s, ctx="match_from")      # one for all: the params' key
                assert list(one[0]) == list(g) and one[0].next == g.next and one[0].total == g.total
            # from[i] replaces match_from: both given, the array wins
            L = N.lib()
            p = L.nxs_params_create()
            L.nxs_params_set_uint(p, b"match_from", M[-1])
            L.nxs_params_set_uint(p, b"match_limit", 4)
            L.nxs_params_set_bool(p, b"fuzzymatch", False)
            out, errs = (C.c_void_p * 2)(), (C.c_int * 2)()
            qs = (C.c_char_p * 2)(q.encode(), q.encode())
            frm = (C.c_uint64 * 2)(M[2], 0)
            assert L.nxs_index_match_docs_batch(gidx._h, p, qs, 2, frm, out, errs) == 0
            assert [list(N._drain_docs(out[i])) for i in range(2)] == [M[2:6], M[:4]]
            assert L.nxs_index_match_docs_batch(gidx._h, p, qs, 2, None, out, errs) == 0
            assert [list(N._drain_docs(out[i])) for i in range(2)] == [[M[-1]], [M[-1]]]
            one = L.nxs_index_match_docs(gidx._h, p, q.encode(), len(q))
            assert list(N._drain_docs(one)) == [M[-1]]
            L.nxs_params_release(p)
    finally:
        gidx.close()


# ---- 4. groups and passes -----------------------------------------------------------------------------------

@ROUTES
def test_groups_and_passes(nxs, small, monkeypatch, route):
    """33 distinct pairs in one batch are two passes; a small NXS_GPU_MATCHDOCS_WS makes groups of one; identical
    pairs are answered once, the same plan with two cursors twice -- all read off the profile"""
    t, d, truth = small
    gidx = nxs.open_files(t, d)
    rng = random.Random(33)
    pairs_key = "device_pairs" if route is None else "host_pairs"
    distinct = []
    while len(distinct) < 33:
        q = random_query(rng, 4)
        if q not in distinct and truth.M(q):
            distinct.append(q)
    try:
        with routed(monkeypatch, gidx, route):
            check(gidx, truth, distinct, limit=11, start=100, ctx="33 pairs")
            prof = gidx.match_docs_profile(reset=True)
            assert prof[pairs_key] == 33 and prof["calls"] == 1 and prof["passes"] == (2 if route is None else 0), prof
            check(gidx, truth, distinct[:32], limit=11, ctx="32 pairs")
            prof = gidx.match_docs_profile(reset=True)
            assert prof[pairs_key] == 32 and prof["passes"] == (1 if route is None else 0), prof
            # identical pairs once; one plan under two cursors twice
            qs = ["v1 OR v2", "v1 OR v2", "v1 OR v2", "v3", "v1 OR v2"]
            starts = [0, 0, 200, 0, 200]
            got = check(gidx, truth, qs, limit=5, start=starts, ctx="duplicates")
            assert list(got[0]) == list(got[1]) and list(got[2]) == list(got[4]) and list(got[0]) != list(got[2])
            prof = gidx.match_docs_profile()
            assert prof[pairs_key] == 3 and prof["ids"] == 15 and [len(g) for g in got] == [5] * 5, prof
        with routed(monkeypatch, gidx, route, ws=1):
            check(gidx, truth, distinct[:5] + [distinct[0]], limit=300, ctx="G = 1")
            prof = gidx.match_docs_profile()
            assert prof[pairs_key] == 5 and prof["passes"] == (5 if route is None else 0), prof
    finally:
        gidx.close()


# ---- 5. leaves, errors, JSON --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def words_corpus(tmp_path_factory):
    rng = random.Random(5)
    words = ["linux", "lint", "unix", "erlang", "python", "kernel", "shell", "driver", "thread", "lynx"]
    docs = [(7 * i + 1, rng.sample(words, 3)) for i in range(400)]
    t, d, _ = nxsfmt.write_index(str(tmp_path_factory.mktemp("words")), "words", docs)
    term_ids = {w.encode(): O.Index(t, d).lookup(w.encode()) for w in words}
    df = {w: sum(1 for _, toks in docs if w in toks) for w in words}
    return t, d, Truth(O.Index(t, d), docs), words, term_ids, df, docs


@ROUTES
def test_leaves_and_json(nxs, words_corpus, monkeypatch, route):
    """fuzzy, prefix and wildcard leaves resolve as a search's; the JSON"""
    t, d, truth, words, term_ids, df, _ = words_corpus
    gidx = nxs.open_files(t, d)
    by_df = lambda ts: sorted(ts, key=lambda w: (-df[w], term_ids[w.encode()]))
    try:
        with routed(monkeypatch, gidx, route):
            # a token that misses the dictionary resolves through the BK walk, exactly as a search's
            check(gidx, truth, ["linus", "linus AND kernel", "pythom OR shel"], limit=9, start=50, fuzzymatch=True, ctx="fuzzy")
            g = gidx.match_docs(["linus"], fuzzymatch=False)[0]
            assert list(g) == [] and g.total == 0 and g.next is None
            for q, kw, exp in (("lin*", {"prefixmatch": True}, by_df([w for w in words if w.startswith("lin")])),
                               ("l*x AND NOT shell", {"wildcardmatch": True}, by_df([w for w in words if re.fullmatch("l.*x", w)])),
                               ("l?n* OR kernel", {"wildcardmatch": True}, by_df([w for w in words if re.fullmatch("l.n.*", w)]))):
                rw = q.replace(q.split()[0], "(" + " OR ".join(exp) + ")", 1)
                assert len(exp) >= 2
                for k, s in ((3, 0), (50, 700), (MATCH_MAX, 0)):
                    g = gidx.match_docs([q], limit=k, start=s, fuzzymatch=False, **kw)[0]
                    check_page(g, truth.page(q, O.BM25, k, s, rewritten=rw), (q, k, s))
            ids, total, nxt = truth.page("linux OR unix", O.BM25, 3, 30)
            text = gidx.match_docs(['linux OR unix'], limit=3, start=30, fuzzymatch=False, json=True)[0]
            assert text == '{"query":"linux OR unix","docs":[%s],"count":3,"total":%d,"next":%d}' % (
                ",".join(map(str, ids)), total, nxt)
            js = json.loads(gidx.match_docs(["linux  OR unix"], limit=MATCH_MAX, fuzzymatch=False, json=True)[0])
            assert js == {"query": "linux  OR unix", "docs": truth.M("linux OR unix"), "count": total, "total": total}
            assert gidx.match_docs([]) == []
    finally:
        gidx.close()


@ROUTES
def test_errors_in_a_batch(nxs, tmp_path, monkeypatch, route):
    """a parse error and a query of 33 live terms are errs[i] with the promised codes and messages, and the rest of
    the batch is answered; the params keys out of range fail the call"""
    rng = random.Random(33)
    rare = ["r%d" % i for i in range(40)]
    docs = [(3 * i + 1, rng.sample(rare, 4)) for i in range(200)]
    t, d, truth = make(tmp_path, "rare", docs)
    gidx = nxs.open_files(t, d)
    with pytest.raises(O.SearchError) as oe:
        truth.M("broken AND")
    try:
        with routed(monkeypatch, gidx, route):
            q32, q33 = " OR ".join(rare[:32]), " OR ".join(rare[:33])
            qs = ["r1 OR r2", "broken AND", q33, "r3", q32, "r4 AND NOT r5"]
            got = gidx.match_docs(qs, limit=10, start=4, fuzzymatch=False)
            assert isinstance(got[1], N.NxsError) and got[1].code == oe.value.code, got[1]
            assert isinstance(got[2], N.NxsError) and got[2].code == LIMIT, got[2]
            for i in (0, 3, 4, 5):
                check_page(got[i], truth.page(qs[i], O.BM25, 10, 4), ("errs", i))
            assert len(got[4]) == 10 and got[4].total > 150
            L = N.lib()
            assert not L.nxs_index_match_docs(gidx._h, None, q33.encode(), len(q33))
            assert gidx.nxs.error() == (LIMIT, "match_docs is not available for a query of more than 32 terms")
            assert not L.nxs_index_match_docs(gidx._h, None, b"broken AND", 10)
            assert gidx.nxs.error()[0] == oe.value.code
            for limit in (0, MATCH_MAX + 1):
                with pytest.raises(N.NxsError) as e:
                    gidx.match_docs(["r3"], limit=limit)
                assert e.value.code == INVALID and "match_limit" in e.value.msg
    finally:
        gidx.close()


# ---- 6. refresh ---------------------------------------------------------------------------------------------

@ROUTES
def test_refresh(nxs, tmp_path, monkeypatch, route):
    """an in-place append and a removal are seen by the next call; a walk goes on from its cursor over the new set"""
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

    def publish(first=False):
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        if not first:
            nxsfmt.publish_in_place(t, d, timg, dimg)
        return Truth(O.Index(t, d), [(e[1], e[2]) for e in ev if e[0] == "add"], [e[1] for e in ev if e[0] == "rm"])
    try:
        with routed(monkeypatch, gidx, route):
            got = check(gidx, publish(first=True), qs, limit=2, ctx="snapshot 0")
            assert list(got[0]) == [10, 20] and got[0].total == 4 and got[0].next == 21 and list(got[1]) == [10, 20]
            ev.append(("rm", 30))
            ev.append(("add", 130, ["apple", "quince", "zebra", "quince"]))
            tr = publish()
            got = check(gidx, tr, qs, limit=2, start=21, ctx="refreshed")
            assert list(got[0]) == [70, 130] and got[0].total == 4 and got[0].next is None and list(got[5]) == [40, 130]
            check(gidx, tr, qs, limit=MATCH_MAX, ctx="refreshed, all")
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 7. in flight, refusals, composition ----------------------------------------------------------------------

def bits(x):
    import struct
    return struct.pack("<f", x)


@ROUTES
def test_between_begin_and_end(nxs, words_corpus, monkeypatch, route):
    """a call between _begin and _end of pipelined batches, a fuzzy batch among them: the batches' responses equal a
    plain run bit for bit, the call's equal the truth"""
    t, d, truth = words_corpus[:3]
    gidx = nxs.open_files(t, d)
    b1 = ["linux OR unix", "kernel AND shell", "python", "driver AND NOT thread"]
    b2 = ["linus OR unix", "pythom", "lynx OR shel"]                      # tokens that miss the dictionary: a fuzzy pass
    mine = ["linux AND unix", "python", "lint OR lynx OR erlang", "kernl OR shell"]
    as_bits = lambda rs: [[(x, bits(v)) for x, v in r] for r in rs]
    try:
        with routed(monkeypatch, gidx, route):
            plain1 = gidx.search_batch(b1, limit=10, fuzzymatch=False, total=True)
            plain2 = gidx.search_batch(b2, limit=10, fuzzymatch=True)
            gidx.search_batch_begin(b1, limit=10, fuzzymatch=False, total=True)
            gidx.search_batch_begin(b2, limit=10, fuzzymatch=True)
            check(gidx, truth, mine, limit=8, start=99, fuzzymatch=True, ctx="in flight")
            r1 = gidx.search_batch_end()
            assert as_bits(r1) == as_bits(plain1) and [x.total for x in r1] == [x.total for x in plain1]
            assert as_bits(gidx.search_batch_end()) == as_bits(plain2)
    finally:
        gidx.close()


@ROUTES
def test_refusals_and_emulated_world(nxs, words_corpus, monkeypatch, route):
    from nxsearch_amd import multi as M
    t, d, truth = words_corpus[:3]
    sh = nxs.open_shard(t, d, 0, 1)
    set_route(monkeypatch, sh, route)
    with pytest.raises(N.NxsError) as e:
        sh.match_docs(["linux"])
    assert e.value.code == INVALID and e.value.msg == "match_docs is not available on a doc shard"
    set_route(monkeypatch, sh, None)
    sh.close()
    # an emulated world of 2: the call is local -- no collective, the whole batch answered here
    gidx = nxs.open_files(t, d)
    try:
        with routed(monkeypatch, gidx, route):
            M.emulate(gidx, 1, 2)
            check(gidx, truth, ["linux OR unix", "kernel", "python AND NOT shell"], limit=6, start=300, ctx="world 2")
            M.emulate(gidx, 0, 0)
    finally:
        gidx.close()


@ROUTES
def test_composition_with_search_docs(nxs, words_corpus, monkeypatch, route):
    """search_docs(q2, match_docs(q1)) is an exact search within the results of q1: docset_truth with S = M(q1)"""
    t, d, truth, words, _, _, docs = words_corpus
    gidx = nxs.open_files(t, d)
    ds = docset_truth.Truth(O.Index(t, d), docs)
    try:
        with routed(monkeypatch, gidx, route):
            for q1, q2 in (("linux OR unix", "kernel OR python"), ("shell AND NOT driver", "lynx"), ("erlang", "erlang OR lint")):
                S = gidx.match_docs([q1], limit=MATCH_MAX, fuzzymatch=False)[0]
                assert list(S) == truth.M(q1) and S.next is None and len(S) > 10
                for limit in (5, 1000):
                    got = gidx.search_docs([q2], list(S), limit=limit, total=True, fuzzymatch=False)[0]
                    docset_truth.check_docs(got, ds.search_docs(q2, O.BM25, limit, set(truth.M(q1))), (q1, q2, limit))
    finally:
        gidx.close()


def test_an_index_that_is_never_asked_runs_no_pass(nxs, words_corpus):
    t, d, truth = words_corpus[:3]
    gidx = nxs.open_files(t, d)
    gidx.search_batch(["linux OR unix", "python"], limit=10, total=True, explain=True)
    gidx.related(["linux"])
    zero = {"device_pairs": 0, "host_pairs": 0, "passes": 0, "ids": 0, "mask_ms": 0.0, "from_ms": 0.0, "count_ms": 0.0,
            "scan_ms": 0.0, "emit_ms": 0.0, "calls": 0}
    assert gidx.match_docs_profile() == zero
    gidx.match_docs(["nosuchterm"], fuzzymatch=False)                      # nothing to list: no pass either
    assert gidx.match_docs_profile() == zero
    gidx.set_profiling(True)
    got = gidx.match_docs(["linux", "linux OR unix"], limit=5, fuzzymatch=False)
    prof = gidx.match_docs_profile(reset=True)
    assert prof["calls"] == 1 and prof["passes"] == 1 and prof["device_pairs"] == 2 and prof["ids"] == 10, prof
    assert all(prof[k] > 0 for k in ("mask_ms", "from_ms", "count_ms", "scan_ms", "emit_ms")), prof
    assert [len(g) for g in got] == [5, 5] and gidx.match_docs_profile() == zero
    gidx.close()
