"""GPU tier (`-m gpu`) for similar documents: Index.doc_terms (nxs_index_doc_terms_batch, nxsgpu_doc_terms:
k_dv_ord / k_dv_scan / k_dv_merge) and Index.similar (nxs_index_similar_batch: a doc leaf resolved by that pass,
spliced as an OR of resolved terms).

Truth is similar_truth.py: the CPU oracle's one-token scores, the docs' tf, the live df, sorted by (-w bits, term
id); for `similar` the rewritten query on the oracle.  Everything is compared in full: terms, order, tf, df, score
bits, matches; doc ids, score bits, order, total, and explanations.  Every test takes both routes: the device
pass and NXS_GPU_DOCTERMS=host."""
import contextlib
import json
import random

import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from explain_truth import check as check_explained
from similar_truth import Truth, check_results, check_vector

pytestmark = pytest.mark.gpu

ROUTES = pytest.mark.parametrize("route", [None, "host"], ids=["device", "host"])
ALGOS = {"BM25": O.BM25, "TF-IDF": O.TF_IDF}
MISSING = 5


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def set_route(monkeypatch, gidx, route, parts=None, ws=None):
    """NXS_GPU_DOCTERMS: None = the device pass, "host" = the host lookups; NXS_GPU_DOCTERMS_PARTS / _WS"""
    for key, v in (("NXS_GPU_DOCTERMS", route), ("NXS_GPU_DOCTERMS_PARTS", parts), ("NXS_GPU_DOCTERMS_WS", ws)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(v))
    gidx.reconfigure()


@contextlib.contextmanager
def routed(monkeypatch, gidx, route, parts=None, ws=None):
    """the body's term vectors take `route`, and only that route: the profile's counters say so"""
    set_route(monkeypatch, gidx, route, parts, ws)
    gidx.doc_terms_profile(reset=True)
    try:
        yield
        prof = gidx.doc_terms_profile()
        took, other = ("device_docs", "host_docs") if route is None else ("host_docs", "device_docs")
        assert prof[took] > 0 and prof[other] == 0, (route, prof)
    finally:
        set_route(monkeypatch, gidx, None)


def make(path, name, docs, removed=()):
    t, d, term_ids = nxsfmt.write_index(str(path), name, docs, removed=removed)
    return t, d, Truth(O.Index(t, d), docs, removed, term_ids)


def check_docs(gidx, truth, docs, algo, k, mindf, ctx=None):
    got = gidx.doc_terms(docs, limit=k, mindf=mindf, algo=algo)
    assert len(got) == len(docs)
    for doc, g in zip(docs, got):
        check_vector(g, truth.rank(doc, ALGOS[algo], k, mindf), (ctx, doc, algo, k, mindf))
    return got


def check_similar(gidx, truth, docs, algo="BM25", limit=10, terms=None, mindf=None, include_self=None, total=False,
                  explain=False, ctx=None):
    """Index.similar against the rewritten queries on the oracle -- and, with include_self, against the plain
    search_batch of the rewritten queries, bit for bit"""
    got = gidx.similar(docs, limit=limit, algo=algo, terms=terms, mindf=mindf, include_self=include_self, total=total,
                       explain=explain)
    assert len(got) == len(docs)
    for doc, g in zip(docs, got):
        c = (ctx, doc, algo, limit, terms, mindf, include_self)
        want, wtotal, q = truth.similar(doc, ALGOS[algo], limit, terms or 8, mindf or 2, bool(include_self))
        check_results(g, want, c)
        if total:
            assert g.total == wtotal, (c, g.total, wtotal)
        if q is None:
            assert list(g) == [] and (not total or g.total == 0), c
        if explain:
            check_explained(g, list(g), truth.ex, q or "", ALGOS[algo], False, c,
                            tokens=truth.ex.tokens(q, False) if q else [])
    return got


# ---- 1. selection sizes ------------------------------------------------------------------------------

SIZES = (1, 31, 32, 33, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def sizes(tmp_path_factory):
    """Doc 1000 + n holds n terms of its own, each once, and so does its twin 2000 + n (equal tf, equal df 2: the
    floats are equal and the term id decides); doc 3000 (and its twin 3001) holds 40 terms with tf growing with
    the term id (the last entries win); the five terms of doc 4000 have df 1; fillers make the idf positive."""
    docs = [(10 + i, ["fill%d" % (i % 7), "pad"]) for i in range(60)]
    for n in SIZES:
        toks = ["s%dx%d" % (n, i) for i in range(n)]
        docs += [(1000 + n, toks), (2000 + n, list(toks))]
    up = [t for i in range(40) for t in ["u%d" % i] * (i + 1)]
    docs += [(3000, up), (3001, list(up)), (4000, ["z%d" % i for i in range(5)])]
    return make(tmp_path_factory.mktemp("sizes"), "sizes", docs)


@ROUTES
@pytest.mark.parametrize("k", [1, 5, 32])
def test_selection_sizes(nxs, sizes, monkeypatch, route, k):
    t, d, truth = sizes
    gidx = nxs.open_files(t, d)
    probe = [1000 + n for n in SIZES] + [3000, 4000, 2257, 10]
    try:
        with routed(monkeypatch, gidx, route, parts=3):
            for algo in ALGOS:
                for mindf in (1, 2):
                    got = check_docs(gidx, truth, probe, algo, k, mindf, "sizes")
                    assert [g.matches for g in got[:len(SIZES)]] == list(SIZES)
                    # equal floats: the term id decides
                    assert [x[0] for x in got[7]] == [b"s257x%d" % i for i in range(min(k, 257))]
                    assert len({x[3] for x in got[7]}) == 1
                    # w grows with the term id: the last entries win
                    assert [x[0] for x in got[8]] == [b"u%d" % (39 - i) for i in range(min(k, 40))]
                    assert got[9].matches == (5 if mindf == 1 else 0) and len(got[9]) == min(k, got[9].matches)
            # every term of doc 4000 has df 1: no expansion at the default mindf, an empty response, total 0
            for explain in (False, True):
                g = gidx.similar([4000, 1001], limit=5, total=True, explain=explain)
                assert list(g[0]) == [] and g[0].total == 0
                assert [x for x, _ in g[1]] == [2001] and g[1].total == 1
            check_similar(gidx, truth, probe, limit=5, terms=k, total=True, ctx="sizes")
            check_similar(gidx, truth, [4000, 3000], limit=5, terms=k, mindf=1, total=True, include_self=True, ctx="sizes")
    finally:
        gidx.close()


# ---- 2. list shapes, 3. negative impacts -----------------------------------------------------------

N_SHAPES = 5003
COUNTS = (1, 2, 63, 64, 65)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """5003 docs (two 4096-doc words), sparse ids with the upper part above 2^32.  `all` is in every doc, `most`
    in 60 % (more than half: see test_list_shapes), `half` in 45 % with one posting of tf 900 in a probed doc (a
    dense column; TF-IDF: beyond the cap), n<k> in exactly k docs, 203 v-words of df ~ 75 each (NXS_GPU_BM_SHARE
    = 64 gives about half of them a bitmap row), and a word of its own per probed doc.  208 + 6 + 12 terms: not
    a multiple of 64."""
    rng = random.Random(5003)
    vocab = ["v%d" % i for i in range(203)]
    members = {k: set(rng.sample(range(N_SHAPES), k)) for k in COUNTS}
    probe_ords = [0, 1, 63, 64, 4095, 4096, N_SHAPES - 1] + sorted(members[2]) + sorted(members[65])[:3]
    docs, did = [], 0
    for i in range(N_SHAPES):
        did += rng.randint(1, 1000)
        if i == 3000:
            did += 1 << 32
        toks = ["all"] * rng.randint(1, 2) + [rng.choice(vocab) for _ in range(rng.randint(1, 5))]
        if rng.random() < 0.6:
            toks.append("most")
        if rng.random() < 0.45 or i == 4096:
            toks += ["half"] * (900 if i == 4096 else rng.randint(1, 3))
        toks += ["n%d" % k for k in COUNTS if i in members[k]] * rng.randint(1, 2)
        if i in probe_ords:
            toks.append("own%d" % i)
        docs.append((did, toks))
    t, d, truth = make(tmp_path_factory.mktemp("shapes"), "shapes", docs)
    assert docs[-1][0] > 1 << 32 and len(truth.term_ids) % 64 != 0
    return t, d, truth, [docs[i][0] for i in probe_ords], docs


def open_shapes(nxs, shapes, monkeypatch):
    monkeypatch.setenv("NXS_GPU_BM_SHARE", "64")
    return nxs.open_files(shapes[0], shapes[1])


@ROUTES
@pytest.mark.parametrize("algo", ["BM25", "TF-IDF"])
def test_list_shapes(nxs, shapes, monkeypatch, route, algo):
    """3. (negative impacts): a term in more than half the docs under BM25.  The reference's BM25 takes
    idf = log((N - df + 0.5) / (df + 0.5) + 1) (ranking.c:171-174, the oracle's orc_bm25), which is positive for
    every df <= N, and its TF-IDF idf is log(N / df) + 1 >= 1: rank() is negative only for tf <= 0 or an average
    doc length below 1, which no live posting has.  So `most` (60 % of the docs) and `all` (every doc) ARE
    eligible by the definition -- w is the oracle's one-token score, >= 0 -- and what is checked is that they come
    with exactly that float, in their place in the order; the w < 0 branch of the kernels cannot be reached from
    an index file."""
    t, d, truth, probe, docs = shapes
    gidx = open_shapes(nxs, shapes, monkeypatch)
    try:
        with routed(monkeypatch, gidx, route):
            for k, mindf in ((5, 1), (32, 1), (8, 2), (32, 70), (32, 80), (3, 3000)):
                check_docs(gidx, truth, probe, algo, k, mindf, "shapes")
            for doc in probe:                                          # a chunk of one doc: a lane per term
                check_docs(gidx, truth, [doc], algo, 32, 1, "shapes one")
            v = gidx.doc_terms([docs[4096][0]], limit=32, algo=algo)[0]
            names = [x[0] for x in v]
            if algo == "BM25":
                for name in (b"all", b"most", b"half"):
                    w = truth.ex.contrib(name, O.BM25)[docs[4096][0]]
                    assert w > 0.0 and v[names.index(name)][3] == w
                assert (b"half", 900) in [(x[0], x[1]) for x in v] and names.index(b"all") > names.index(b"most")
            else:
                # the regular posting's uncapped float: tf 900, the term's largest impact by far
                w = truth.ex.contrib(b"half", O.TF_IDF)
                row = v[names.index(b"half")]
                assert row[1] == 900 and row[3] == w[docs[4096][0]] == max(w.values())
                assert row[3] > 2 * sorted(w.values())[-2]
            check_similar(gidx, truth, probe, algo=algo, limit=10, total=True, ctx="shapes")
            check_similar(gidx, truth, probe[:6], algo=algo, limit=10, terms=32, mindf=1, explain=True, ctx="shapes")
    finally:
        gidx.close()


@ROUTES
def test_a_dictionary_of_one_term(nxs, tmp_path, monkeypatch, route):
    docs = [(7, ["only"]), (9, ["only", "only"]), (1 << 40, ["only"] * 3)]
    t, d, truth = make(tmp_path, "one", docs)
    gidx = nxs.open_files(t, d)
    try:
        with routed(monkeypatch, gidx, route):
            got = check_docs(gidx, truth, [7, 9, 1 << 40], "TF-IDF", 5, 1, "one")
            assert [[x[:3] for x in g] for g in got] == [[(b"only", 1, 3)], [(b"only", 2, 3)], [(b"only", 3, 3)]]
            got = check_docs(gidx, truth, [7, 9, 1 << 40], "BM25", 5, 1, "one")
            assert [g.matches for g in got] == [1, 1, 1] and all(g[0][3] > 0.0 for g in got)
            got = check_docs(gidx, truth, [7, 9, 1 << 40], "BM25", 5, 4, "one")      # df 3 < mindf 4
            assert [list(g) for g in got] == [[], [], []] and [g.matches for g in got] == [0, 0, 0]
            check_similar(gidx, truth, [7, 9], algo="TF-IDF", limit=2, total=True, ctx="one")
            check_similar(gidx, truth, [7, 9], algo="BM25", limit=2, total=True, ctx="one")
    finally:
        gidx.close()


# ---- 4. batches ---------------------------------------------------------------------------------------

@ROUTES
@pytest.mark.parametrize("parts,ws", [(None, None), (1, None), (2, 1)], ids=["default", "one-part", "many-passes"])
def test_batches(nxs, shapes, monkeypatch, route, parts, ws):
    """1, 64, 65 and 300 docs with duplicates and an id that is not a live doc in the middle; NXS_GPU_DOCTERMS_WS
    = 1 cuts the batch into passes of one chunk each"""
    t, d, truth, probe, docs = shapes
    rng = random.Random(300)
    gidx = open_shapes(nxs, shapes, monkeypatch)
    bad = docs[100][0] + 1 if docs[100][0] + 1 != docs[101][0] else docs[100][0] - 1
    assert bad not in truth.of_doc
    try:
        with routed(monkeypatch, gidx, route, parts, ws):
            for n in (1, 64, 65, 300):
                ids = [docs[rng.randrange(N_SHAPES)][0] for _ in range(n)]
                ids[n // 3] = ids[0]                                    # a duplicate
                if n > 1:
                    ids[n // 2] = bad
                    ids[-1] = ids[1]
                got = gidx.doc_terms(ids, limit=8, mindf=2)
                for i, (doc, g) in enumerate(zip(ids, got)):
                    if doc == bad:
                        assert isinstance(g, N.NxsError) and g.code == MISSING, (n, i)
                    else:
                        check_vector(g, truth.rank(doc, O.BM25, 8, 2), ("batch", n, i, doc))
                assert got[n // 3] == got[0] and got[n // 3].matches == got[0].matches
                sim = gidx.similar(ids, limit=5, total=True)
                for i, (doc, g) in enumerate(zip(ids, sim)):
                    if doc == bad:
                        assert isinstance(g, N.NxsError) and g.code == MISSING, (n, i)
                    else:
                        want, wtotal, _ = truth.similar(doc, O.BM25, 5)
                        check_results(g, want, ("similar batch", n, i, doc))
                        assert g.total == wtotal
            if route is None and ws:
                prof = gidx.doc_terms_profile()
                assert prof["passes"] > prof["calls"], prof             # the 300-doc batches took several passes
            # a batch of searches in flight around a batch of docs: both are right
            qs = ["v1 OR v2", "half AND v3", "n65", "all AND NOT most"]
            plain = gidx.search_batch(qs, limit=10, fuzzymatch=False)
            gidx.search_batch_begin(qs, limit=10, fuzzymatch=False)
            check_docs(gidx, truth, probe, "BM25", 8, 1, "in flight")
            assert gidx.search_batch_end() == plain
            # one call, one doc
            L = N.lib()
            sg = L.nxs_index_doc_terms(gidx._h, None, probe[0])
            assert sg
            check_vector(N._drain_docterms(sg), truth.rank(probe[0], O.BM25, 5, 1), "single")
            assert not L.nxs_index_doc_terms(gidx._h, None, bad) and nxs.error() == (MISSING, "no such document")
            assert not L.nxs_index_similar(gidx._h, None, bad) and nxs.error() == (MISSING, "no such document")
            assert gidx.doc_terms([]) == [] and gidx.similar([]) == []
    finally:
        gidx.close()


# ---- 5. snapshots -------------------------------------------------------------------------------------

@ROUTES
def test_snapshots(nxs, tmp_path, monkeypatch, route):
    ev = [("add", 10, ["apple", "maple", "zebra"]), ("add", 20, ["apple", "apply", "pear"]),
          ("add", 30, ["ample", "apple", "pear"]), ("add", 40, ["apply", "zebra"]), ("add", 50, ["ample", "fig"]),
          ("add", 60, ["apricot", "fig"]), ("add", 70, ["kiwi"]), ("add", 80, ["lime", "kiwi"]), ("add", 90, ["plum"]),
          ("add", 100, ["plum", "lime"]), ("add", 110, ["date"]), ("add", 120, ["date", "sloe"]), ("rm", 60)]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 262144)
    open(d, "wb").write(dimg + b"\0" * 262144)
    gidx = nxs.open_files(t, d)

    def truth_now():
        docs = [(e[1], e[2]) for e in ev if e[0] == "add"]
        removed = [e[1] for e in ev if e[0] == "rm"]
        _, _, term_ids = nxsfmt.build_images_log(ev)
        return Truth(O.Index(t, d), docs, removed, term_ids)

    def publish():
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        nxsfmt.publish_in_place(t, d, timg, dimg)
        return truth_now()

    def check_all(truth, ctx):
        live = truth.live
        for algo in ALGOS:
            check_docs(gidx, truth, live, algo, 5, 1, ctx)
            check_similar(gidx, truth, live, algo=algo, limit=3, total=True, ctx=ctx)
        return gidx.doc_terms(live + [60], limit=5)
    try:
        with routed(monkeypatch, gidx, route):
            truth = truth_now()
            got = check_all(truth, "snapshot 0")
            assert isinstance(got[-1], N.NxsError) and got[-1].code == MISSING           # removed before the open
            assert b"apply" in truth.expansions(40, O.BM25) and (b"fig", 1, 1) in [x[:3] for x in got[truth.live.index(50)]]
            ev.append(("rm", 20))                                      # "apply" falls to df 1, "apple" to 2
            truth = publish()
            got = gidx.doc_terms([20, 40], limit=5)
            assert isinstance(got[0], N.NxsError) and got[0].code == MISSING
            assert (b"apply", 1, 1) in [x[:3] for x in got[1]]
            assert b"apply" not in truth.expansions(40, O.BM25) and truth.expansions(40, O.BM25) == [b"zebra"]
            check_all(truth, "removal")
            assert [x for x, _ in gidx.similar([40], limit=3)[0]] == [10]
            ev.append(("add", 130, ["apply", "quince", "zebra", "quince"]))       # a new doc with a new term
            truth = publish()
            got = check_all(truth, "append")
            assert (b"quince", 2, 1) in [x[:3] for x in got[truth.live.index(130)]]
            assert 130 in [x for x, _ in gidx.similar([40], limit=3)[0]]
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 6. `similar` semantics ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sem(tmp_path_factory):
    """900 docs over a 60-word vocabulary; doc 5 is long (every word, many times) and many short docs score
    better on its expansions under BM25 (a word of its own makes it longer still)"""
    rng = random.Random(900)
    vocab = ["w%d" % i for i in range(60)]
    weights = [1.0 / (i + 3) for i in range(60)]
    docs = [(5, [w for w in vocab for _ in range(20)] + ["padpad"] * 3000)]
    did = 5
    for _ in range(900):
        did += rng.randint(1, 50)
        docs.append((did, rng.choices(vocab, weights, k=rng.randint(1, 6))))
    return make(tmp_path_factory.mktemp("sem"), "sem", docs) + (docs,)


@ROUTES
def test_similar_semantics(nxs, sem, monkeypatch, route):
    t, d, truth, docs = sem
    gidx = nxs.open_files(t, d)
    rng = random.Random(6)
    probe = [5] + [docs[rng.randrange(1, len(docs))][0] for _ in range(24)]
    try:
        with routed(monkeypatch, gidx, route):
            for algo in ALGOS:
                for terms in (1, 8, 32):
                    # include_self: the plain search of the rewritten query, bit for bit
                    got = check_similar(gidx, truth, probe, algo=algo, limit=10, terms=terms, include_self=True, total=True,
                                        ctx="self")
                    qs = [truth.rewritten(doc, ALGOS[algo], terms, 2) for doc in probe]
                    assert all(qs)
                    plain = gidx.search_batch(qs, limit=10, algo=algo, fuzzymatch=False, total=True)
                    for g, p in zip(got, plain):
                        check_results(g, list(p), ("vs search_batch", algo, terms))
                        assert g.total == p.total
                    # the default drops the source: total == the rewritten query's - 1
                    drop = check_similar(gidx, truth, probe, algo=algo, limit=10, terms=terms, total=True, ctx="drop")
                    for doc, g, p in zip(probe, drop, plain):
                        assert doc not in [x for x, _ in g] and g.total == p.total - 1
                    check_similar(gidx, truth, probe[:8], algo=algo, limit=10, terms=terms, explain=True, total=True,
                                  ctx="explain")
                    check_similar(gidx, truth, probe[:8], algo=algo, limit=10, terms=terms, explain=True,
                                  include_self=True, ctx="explain self")
            # the source is not in the top limit + 1: the long doc under BM25 -- the last result goes
            eleven = gidx.search_batch([truth.rewritten(5, O.BM25)], limit=11, fuzzymatch=False)[0]
            assert 5 not in [x for x, _ in eleven] and len(eleven) == 11
            assert list(gidx.similar([5], limit=10)[0]) == list(eleven)[:10]
            # a limit above the docs there are (the exact path), explained
            check_similar(gidx, truth, probe[:4], limit=1000, explain=True, total=True, ctx="limit 1000")
            check_similar(gidx, truth, probe[:4], limit=9000, total=True, ctx="limit 9000")
            # ignored keys; params out of range name their key
            for lim, key, kw in ((0, "similar_terms", "terms"), (33, "similar_terms", "terms"), (0, "similar_mindf", "mindf")):
                with pytest.raises(N.NxsError) as e:
                    gidx.similar([5], **{kw: lim})
                assert e.value.code == 3 and key in e.value.msg
            for key, kw, bad in (("docterms_limit", "limit", (0, 33)), ("docterms_mindf", "mindf", (0,))):
                for v in bad:
                    with pytest.raises(N.NxsError) as e:
                        gidx.doc_terms([5], **{kw: v})
                    assert e.value.code == 3 and key in e.value.msg
            with pytest.raises(N.NxsError) as e:
                gidx.similar([5], limit=(1 << 32) - 1)
            assert e.value.code == 3 and e.value.msg == "invalid limit"
            # the JSON of a term vector
            js = json.loads(gidx.doc_terms([probe[1]], limit=3, json=True)[0])
            want, m = truth.rank(probe[1], O.BM25, 3, 1)
            assert list(js) == ["doc_id", "terms", "matches"] and js["doc_id"] == probe[1] and js["matches"] == m
            assert [(x["term"].encode(), x["tf"], x["df"], x["score"]) for x in js["terms"]] == want
    finally:
        gidx.close()


@ROUTES
def test_doc_shards_are_refused_and_an_emulated_world_serves_its_slice(nxs, sem, monkeypatch, route):
    from nxsearch_amd import multi
    t, d, truth, docs = sem
    sh = nxs.open_shard(t, d, 0, 1)
    set_route(monkeypatch, sh, route)
    with pytest.raises(N.NxsError) as e:
        sh.doc_terms([5])
    assert e.value.code == 3 and e.value.msg == "doc_terms is not available on a doc shard"
    with pytest.raises(N.NxsError) as e:
        sh.similar([5])
    assert e.value.code == 3 and e.value.msg == "similar is not available on a doc shard"
    sh.close()
    gidx = nxs.open_files(t, d)
    probe = [docs[i][0] for i in range(0, 40, 3)]
    try:
        with routed(monkeypatch, gidx, route):
            whole = gidx.similar(probe, limit=10, explain=True)
            covered = 0
            for rank in range(2):
                multi.emulate(gidx, rank, 2)
                lo, hi = multi.shard_slice(len(probe), rank, 2)
                got = gidx.similar(probe, limit=10, explain=True)
                for i, (g, w) in enumerate(zip(got, whole)):
                    if lo <= i < hi:
                        check_results(g, list(w), ("emulated", rank, i))
                        assert g.tokens == w.tokens and g.explain == w.explain
                        covered += 1
                    else:
                        assert isinstance(g, N.NxsError), (rank, i)     # another rank's slice: not held here
                with pytest.raises(N.NxsError) as e:
                    gidx.similar(probe, limit=10, total=True)
                assert e.value.code == 3 and e.value.msg == "total is not available on a sharded batch"
                # a term vector is local: every rank answers its own calls
                check_docs(gidx, truth, probe, "BM25", 5, 1, "emulated")
            assert covered == len(probe)
            multi.emulate(gidx, 0, 0)
            check_similar(gidx, truth, probe, limit=10, total=True, ctx="after")
    finally:
        multi.emulate(gidx, 0, 0)
        gidx.close()


def test_an_index_that_is_never_asked_runs_no_pass(nxs, sem):
    t, d, truth, docs = sem
    gidx = nxs.open_files(t, d)
    gidx.search_batch(["w1 OR w2", "w3"], limit=10, total=True, explain=True)
    assert gidx.doc_terms_profile() == {"calls": 0, "ord_ms": 0.0, "scan_ms": 0.0, "merge_ms": 0.0, "passes": 0,
                                        "device_docs": 0, "host_docs": 0, "eligible": 0}
    gidx.set_profiling(True)
    got = gidx.doc_terms([5, 5, docs[1][0]], limit=32)
    prof = gidx.doc_terms_profile(reset=True)
    assert prof["calls"] == 1 and prof["passes"] == 1 and prof["device_docs"] == 2 and prof["scan_ms"] > 0, prof
    assert prof["eligible"] == got[0].matches + got[2].matches and got[0] == got[1]
    assert gidx.doc_terms_profile()["calls"] == 0
    gidx.close()
