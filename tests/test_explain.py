"""GPU tier (`-m gpu`) for explanations: params "explain" -> nxs_resp_tokens / _token / _explain.

Truth is the CPU oracle and the docs a test wrote (explain_truth.py).  Every checked result demands: ids and
score bits equal to the same call without "explain", the token list (order, duplicates), presence per (result,
token), the oracle's contribution bits, the docs' tf, and the f32 sum in ascending token order equal to the
returned score bit for bit.  Every query of every list is compared."""
import random
import shutil

import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from complete_truth import big_corpus, docs_of, rewrite, truth_of_docs
from explain_truth import Truth, check, tf_of_docs, tf_of_dtmap, tf_of_events
from nxsearch_amd import corpus

pytestmark = pytest.mark.gpu

ALGOS = {"BM25": (O.BM25, "BM25"), "TF-IDF": (O.TF_IDF, "TF-IDF")}
NO_MATCH = "qqqqqqqqqqqqqqqq"       # beyond the fuzzy tolerance of every term of every test dictionary


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def check_batch(gidx, truth, qs, ctx, limit=10, algo="BM25", fuzzymatch=False, **kw):
    """search_batch with and without explain; -> present cells"""
    plain = gidx.search_batch(qs, limit=limit, algo=algo, fuzzymatch=fuzzymatch, **kw)
    got = gidx.search_batch(qs, limit=limit, algo=algo, fuzzymatch=fuzzymatch, explain=True, **kw)
    assert len(got) == len(qs)
    return sum(check(g, p, truth, q, ALGOS[algo][0], fuzzymatch, (ctx, limit, algo)) for q, g, p in zip(qs, got, plain))


def random_query(rng, vocab, nmax):
    q = rng.choice(vocab)
    for _ in range(rng.randint(1, nmax) - 1):
        q += rng.choice([" AND ", " OR ", " AND NOT ", " "]) + rng.choice(vocab)
    return q


# ---- list and ordinal edges ---------------------------------------------------------------------------

N_EDGE = 8193
EDGE_ORDS = (0, 63, 64, 4095, 4096, 8192)
EDGE_COUNTS = (1, 2, 63, 64, 65)


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    """8193 docs, sparse ids (the upper third above 2^32): `all` in every doc (dense column, bitmap row), n<k>
    with exactly k postings (k >= 8 gets a bitmap row, 1 and 2 do not), o<i> only in ordinal i, fillers."""
    rng = random.Random(8193)
    vocab = ["v%d" % i for i in range(10)]
    members = {k: set(rng.sample(range(N_EDGE), k)) for k in EDGE_COUNTS}
    docs, did = [], 0
    for i in range(N_EDGE):
        did += rng.randint(1, 1000)
        if i == 5500:
            did += 1 << 32
        toks = ["all"] * rng.randint(1, 3) + [rng.choice(vocab) for _ in range(rng.randint(0, 3))]
        toks += ["n%d" % k for k in EDGE_COUNTS if i in members[k]] * rng.randint(1, 2)
        toks += ["o%d" % o for o in EDGE_ORDS if o == i]
        docs.append((did, toks))
    t, d, _ = nxsfmt.write_index(str(tmp_path_factory.mktemp("edge")), "edge", docs)
    truth = Truth(O.Index(t, d), tf_of_docs(docs))
    assert docs[-1][0] > 1 << 32 and len(truth.contrib("all", O.BM25)) == N_EDGE
    for k in EDGE_COUNTS:
        assert len(truth.contrib("n%d" % k, O.BM25)) == k
    for o in EDGE_ORDS:
        assert list(truth.contrib("o%d" % o, O.BM25)) == [docs[o][0]]
    return t, d, truth


def edge_queries():
    rng = random.Random(5)
    ns, os_ = ["n%d" % k for k in EDGE_COUNTS], ["o%d" % o for o in EDGE_ORDS]
    qs = ["all"] + ns + os_
    qs += [" OR ".join(os_), " OR ".join(ns), "all AND n63", "all AND n64 AND n65", "n65 AND NOT n64", "all AND NOT n65",
           "o0 OR o8192", "o63 OR o64", "o4095 OR o4096", "all AND o4096", "all AND (o63 OR o64 OR o8192)",
           "(n1 OR n2) AND all", "n64 OR o64 OR v1", "v1 AND v2", "v3 OR v4 OR n2", "v5 AND NOT all",
           "all AND NOT (o0 OR o8192)", "n63 AND n64"]
    vocab = ["v%d" % i for i in range(10)] + ns + os_ + ["all"]
    return qs + [random_query(rng, vocab, 5) for _ in range(12)]


@pytest.mark.parametrize("rows", [None, 100], ids=["rows-default", "rows-100"])
@pytest.mark.parametrize("algo", ["BM25", "TF-IDF"])
def test_list_and_ordinal_edges(nxs, edge, monkeypatch, algo, rows):
    t, d, truth = edge
    if rows:
        monkeypatch.setenv("NXS_GPU_EXPLAIN_ROWS", str(rows))
    gidx = nxs.open_files(t, d)
    qs = edge_queries()
    cells = 0
    for limit in (1, 10, 64, 65, 1000):
        cells += check_batch(gidx, truth, qs, "edge", limit=limit, algo=algo)
    # the exact path: every matching doc is returned (a third of the list: 8193 rows a query)
    cells += check_batch(gidx, truth, qs[:1] + qs[12:24:2], "edge exact", limit=9000, algo=algo)
    prof = gidx.explain_profile()
    assert prof["passes"] == 6 and prof["present"] == cells and prof["cells"] >= cells, prof
    if rows:
        assert prof["chunks"] >= prof["cells"] // rows > 6, prof     # many chunks, same answers
    else:
        assert prof["chunks"] == prof["passes"], prof
    gidx.close()


# ---- token-list shapes --------------------------------------------------------------------------------

def test_token_list_shapes(nxs, tmp_path):
    """1, 8, 9, 32 and 33 tokens (33: the wide plan); one term reached through two strings (Q6: it adds twice); a
    token under NOT that the doc holds through another branch; an unresolved token; queries that match nothing."""
    rng = random.Random(33)
    vocab = ["w%d" % i for i in range(40)]
    names = ["linux", "unix", "kernel", "shell"]
    weights = [1.0 / (i + 2) for i in range(len(vocab))]
    docs, did = [], 0
    for _ in range(4000):
        did += rng.randint(1, 9)
        docs.append((did, rng.choices(vocab, weights, k=rng.randint(1, 12)) + rng.sample(names, rng.randint(0, 2))))
    docs.append((did + 1, ["w1", "w3", "w1"]))          # holds a and c of `a OR (b AND NOT c)`
    t, d, _ = nxsfmt.write_index(str(tmp_path), "shapes", docs)
    oidx = O.Index(t, d)
    gidx, truth = nxs.open_files(t, d), Truth(oidx, tf_of_docs(docs))
    qs = [" OR ".join(vocab[:k]) for k in (1, 8, 9, 32, 33)]
    qs += ["(" + " OR ".join(vocab[:20]) + ") AND (" + " OR ".join(vocab[20:33]) + ")",
           " ".join(vocab[5:14]) + " AND NOT w0", " AND ".join(vocab[:3]) + " AND (" + " OR ".join(vocab[3:36]) + ")"]
    qs += ["linus OR linuz", "linus AND linuz", "linus OR linuz OR unix", "linus linuz linvx", "linux OR linus",
           "(linus OR w2) AND linuz"]
    qs += ["w1 OR (w2 AND NOT w3)", "w0 AND NOT w1", "(w0 AND NOT w1) OR (w1 AND NOT w0)", "w1 OR w1", "w2 AND w2 AND w1"]
    qs += ["w1 OR " + NO_MATCH, NO_MATCH + " OR w2 OR " + NO_MATCH, "w1 AND " + NO_MATCH, NO_MATCH, "w1 AND NOT w1"]
    # what the shapes rest on, from the oracle
    assert oidx.fuzzy(b"linus")[0] == oidx.fuzzy(b"linuz")[0] == oidx.lookup(b"linux") != 0
    assert truth.tokens("linus OR linuz", True) == [b"linux", b"linux"]
    assert truth.tokens("w1 OR " + NO_MATCH, True) == [b"w1"] and truth.tokens(NO_MATCH, True) == []
    assert len(truth.tokens(qs[4], True)) == 33 and truth.tokens("w1 OR w1", True) == [b"w1"]
    assert not oidx.search("w1 AND NOT w1") and not oidx.search(NO_MATCH)
    for algo in ALGOS:
        for limit in (10, 1000):
            check_batch(gidx, truth, qs, "shapes", limit=limit, algo=algo, fuzzymatch=True)
    # the doc with a and c: c stands under NOT, the doc holds it, so it contributes
    g = gidx.search("w1 OR (w2 AND NOT w3)", limit=5000, explain=True)
    row = g.explain[[doc for doc, _ in g].index(did + 1)]
    assert g.tokens == [b"w3", b"w2", b"w1"] and [(j, tf) for j, tf, _ in row] == [(0, 1), (2, 2)]
    # one query (the blocking search) and its JSON
    import json
    doc = json.loads(gidx.search("linus OR linuz", limit=3, explain=True, json=True))
    assert doc["tokens"] == ["linux", "linux"] and doc["count"] == 3
    for r, (_, score) in zip(doc["results"], gidx.search("linus OR linuz", limit=3)):
        assert [x["t"] for x in r["terms"]] == [0, 1] and r["terms"][0] == dict(r["terms"][1], t=0)
        assert r["score"] == score
    assert json.loads(gidx.search(NO_MATCH, explain=True, json=True)) == {"results": [], "count": 0, "tokens": []}
    assert "tokens" not in json.loads(gidx.search("w1", limit=2, json=True))
    gidx.close()


# ---- TF-IDF outlier lists -----------------------------------------------------------------------------

def test_tfidf_outliers_report_the_full_impact(nxs, tmp_path, monkeypatch):
    """A dense term with a few postings of a very large tf: under TF-IDF its ceiling is capped and those
    postings form an outlier list holding impact - cap.  The explanation reports the full impact."""
    monkeypatch.setenv("NXS_GPU_DROP_MINPOST", "1")     # the sparse + dense class for every eligible query
    rng = random.Random(77)
    vocab = ["s%d" % i for i in range(300)]
    docs, big = [], set(rng.sample(range(6000), 12))
    for i in range(6000):
        # (the outlier docs also hold s0..s39: they lead every OR query below)
        docs.append((3 * i + 1, ["dense"] * (400 if i in big else rng.randint(1, 3)) +
                     (vocab[:40] if i in big else rng.sample(vocab, 2))))
    t, d, _ = nxsfmt.write_index(str(tmp_path), "outl", docs)
    gidx, truth = nxs.open_files(t, d), Truth(O.Index(t, d), tf_of_docs(docs))
    qs = ["dense OR s%d OR s%d" % (i, i + 1) for i in range(0, 40, 2)] + ["dense", "dense AND s1", "s2 OR dense"]
    gidx.set_profiling(True)
    gidx.profile(reset=True)
    for limit in (10, 64, 1000):
        check_batch(gidx, truth, qs, "outliers", limit=limit, algo="TF-IDF")
    kinds = {c["key"] >> 8 for c in gidx.profile(reset=True)["classes"]}
    assert kinds & {5, 9}, kinds                        # the dense term left the scan: cap + outlier list in use
    gidx.set_profiling(False)
    # the outlier docs lead every such query, and their `dense` cell is the oracle's full float
    m = truth.contrib("dense", O.TF_IDF)
    top = sorted(m.values())[-12]
    assert top > 3 * sorted(m.values())[-13]
    g = gidx.search("dense OR s0 OR s1", limit=12, algo="TF-IDF", explain=True, fuzzymatch=False)
    assert {doc for doc, _ in g} == {3 * i + 1 for i in big}
    for (doc, _), row in zip(g, g.explain):
        j, tf, s = row[-1]
        assert g.tokens[j] == b"dense" and tf == 400 and s == m[doc] >= top
    check_batch(gidx, truth, qs, "outliers", limit=10, algo="BM25")
    gidx.close()


# ---- fuzzy and prefix ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big(nxs, tmp_path_factory):
    term_dfs, dead, words = big_corpus()
    docs, removed = docs_of(term_dfs, dead)
    t, d, term_ids = nxsfmt.write_index(str(tmp_path_factory.mktemp("big")), "big", docs, removed=removed)
    gidx = nxs.open_files(t, d)
    yield gidx, Truth(O.Index(t, d), tf_of_docs(docs, removed)), truth_of_docs(docs, removed, term_ids), words
    gidx.close()


def test_fuzzy_tokens_name_the_oracles_winner(big):
    gidx, truth, _, words = big
    rng = random.Random(404)
    have = set(words)
    live = words[:1940]

    def misspell(w):
        while True:
            b = bytearray(w)
            b[rng.randrange(len(b))] = ord(rng.choice("abcdefgh"))
            if bytes(b) not in have:
                return bytes(b).decode()
    qs = []
    for _ in range(60):
        ws = [rng.choice(live).decode() for _ in range(rng.randint(1, 4))]
        k = rng.randrange(len(ws))
        ws[k] = misspell(ws[k].encode())
        qs.append(rng.choice([" OR ", " AND ", " "]).join(ws))
    qs += [misspell(live[7]), misspell(words[1950]) + " OR " + live[3].decode(), NO_MATCH + " OR " + misspell(live[9])]
    resolved = [truth.tokens(q, True) for q in qs]
    assert sum(len(r) for r in resolved) > 100
    for algo in ALGOS:
        for limit in (10, 1000):
            check_batch(gidx, truth, qs, "fuzzy", limit=limit, algo=algo, fuzzymatch=True)


@pytest.mark.parametrize("pl", [1, 8, 32])
def test_prefix_leaves_are_explained_as_their_expansions(big, pl):
    gidx, truth, ptruth, words = big
    rng = random.Random(500 + pl)
    live = words[:1940]
    qs = []
    for _ in range(40):
        w = rng.choice(live)
        p = w[:rng.randint(1, min(3, len(w)))].decode() + "*"
        others = [rng.choice(live).decode() for _ in range(rng.randint(0, 3))]
        parts = others + [p]
        rng.shuffle(parts)
        qs.append(rng.choice([" OR ", " AND ", " "]).join(parts))
    qs += ["a* OR b*", "ab* AND NOT a", "f*", "(a* AND b*) OR " + live[5].decode(), NO_MATCH[:6] + "* OR " + live[6].decode()]
    for algo in ALGOS:
        for limit in (10, 1000):
            plain = gidx.search_batch(qs, limit=limit, algo=algo, fuzzymatch=False, prefixmatch=True, prefix_limit=pl)
            got = gidx.search_batch(qs, limit=limit, algo=algo, fuzzymatch=False, prefixmatch=True, prefix_limit=pl,
                                    explain=True)
            for q, g, p in zip(qs, got, plain):
                r = rewrite(q, ptruth, pl, lowercase=False)
                check(g, p, truth, q, ALGOS[algo][0], False, ("prefix", pl, limit, algo, r[:80]),
                      tokens=truth.tokens(r, False))
    if pl == 32:
        assert max(len(truth.tokens(rewrite(q, ptruth, pl, lowercase=False), False)) for q in qs) > 32    # a wide plan


# ---- pipelining and refresh ---------------------------------------------------------------------------

def test_pipelined_batches_and_refresh_explain_their_own_snapshot(nxs, tmp_path):
    """Four batches in flight, asking and not asking; between two _begins docs are appended and two removed --
    every idf moves, so an explanation taken from the wrong snapshot misses the contribution bits and the
    sum.  `gone` loses all its docs; the last batches' misspelt tokens leave their fuzzy halves pending."""
    rng = random.Random(91)
    vocab = ["cat", "dog", "owl", "emu", "gnu", "yak"] + ["w%d" % i for i in range(12)]
    ev = [("add", 10 * (i + 1), [rng.choice(vocab) for _ in range(rng.randint(1, 6))] + ["cat"] * (i % 3)) for i in range(1500)]
    ev.append(("add", 15007, ["gone", "cat", "gone"]))
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 524288)
    open(d, "wb").write(dimg + b"\0" * 524288)
    gidx = nxs.open_files(t, d)
    snaps = []

    def snapshot():                                     # (a private copy: the oracle reads the header live)
        k = len(snaps)
        tt, dd = str(tmp_path / ("t%d" % k)), str(tmp_path / ("d%d" % k))
        shutil.copy(t, tt)
        shutil.copy(d, dd)
        snaps.append(Truth(O.Index(tt, dd), tf_of_events(ev)))
        return snaps[-1]

    def publish():
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        nxsfmt.publish_in_place(t, d, timg, dimg)
        return snapshot()
    exact = [random_query(rng, vocab, 5) for _ in range(40)] + ["gone OR cat", "gone", "gone AND cat", "cat AND NOT gone"]
    fuzzy = ["caat OR dog", "owl AND doog", "emv gnu", "yak OR yakk OR w1", "gome OR cat"] + exact[:20]
    s0 = snapshot()
    plan = [(exact, True, False), (exact[::-1], False, False), (fuzzy, True, True),                           # snapshot 0
            (exact, True, False), (fuzzy, False, True), (fuzzy[::-1], True, True), (exact[::-1], True, False)]  # snapshot 1
    want, inflight, done = [], [], []

    def end():
        i = inflight.pop(0)
        qs, ask, fz = plan[i]
        got = gidx.search_batch_end()
        assert len(got) == len(qs)
        done.append((i, got))
    for i, (qs, ask, fz) in enumerate(plan):
        if i == 3:
            # three batches of snapshot 0 are in flight, the last with its fuzzy half still pending: the files
            # move, and the next _begin finishes them early -- explained then, before the index follows
            for k in range(40):
                ev.append(("add", 20000 + k, ["cat", "emu", "hen"] + [rng.choice(vocab)]))
            ev.append(("rm", 15007))                    # the only doc of `gone`
            ev.append(("rm", 20))
            s1 = publish()
        gidx.search_batch_begin(qs, limit=10, fuzzymatch=fz, explain=ask)
        want.append(s0 if i < 3 else s1)
        inflight.append(i)
        if len(inflight) == 4:
            end()
    while inflight:
        end()
    assert [i for i, _ in done] == list(range(len(plan)))
    assert s0.contrib("gone", O.BM25) and not s1.contrib("gone", O.BM25) and s1.oidx.lookup(b"gone")
    assert s0.contrib("cat", O.BM25) != s1.contrib("cat", O.BM25)
    for i, got in done:
        qs, ask, fz = plan[i]
        truth = want[i]
        for q, g in zip(qs, got):
            p = truth.oidx.search(q, limit=10, fuzzymatch=fz)
            if ask:
                check(g, p, truth, q, O.BM25, fz, ("pipeline", i))
            else:
                assert [x for x, _ in g] == [x for x, _ in p] and getattr(g, "tokens", None) is None, (i, q)
    # the term without docs sits in the token list and is absent everywhere
    g = gidx.search("gone OR cat", limit=10, fuzzymatch=False, explain=True)
    assert g.tokens == [b"cat", b"gone"] and all([j for j, _, _ in row] == [0] for row in g.explain) and len(g) == 10
    assert gidx.host_profile()["fuzzy_launch_ms"] > 0
    gidx.close()


# ---- random -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rnd(nxs, tmp_path_factory):
    c = corpus.write_corpus(str(tmp_path_factory.mktemp("rnd")), 50_000, 3000, seed=29)
    terms = corpus.term_strings(3000, seed=29)
    rng = random.Random(12)
    ranks = sorted(set([1, 2, 3, 5, 8] + rng.sample(range(1, 2500), 75)))
    vocab = [terms[r - 1].decode() for r in ranks]
    qs = [random_query(rng, vocab, 6) for _ in range(200)]
    truth = Truth(O.Index(c["terms"], c["dtmap"]), tf_of_dtmap(c["dtmap"], terms, ranks))
    gidx = nxs.open_files(c["terms"], c["dtmap"])
    yield gidx, truth, qs
    gidx.close()


@pytest.mark.parametrize("limit", [10, 1000])
@pytest.mark.parametrize("algo", ["BM25", "TF-IDF"])
def test_random_queries(rnd, algo, limit):
    gidx, truth, qs = rnd
    assert check_batch(gidx, truth, qs, "random", limit=limit, algo=algo) > len(qs)


# ---- sharded ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shard_corpus(tmp_path_factory):
    rng = random.Random(61)
    vocab = ["w%d" % i for i in range(50)]
    weights = [1.0 / (i + 1) for i in range(len(vocab))]
    docs, did = [], 0
    for _ in range(9000):
        did += rng.randint(1, 1000)
        docs.append((did, rng.choices(vocab, weights, k=rng.randint(1, 7))))
    t, d, _ = nxsfmt.write_index(str(tmp_path_factory.mktemp("whole")), "whole", docs)
    qs = [random_query(rng, vocab[:16], 5) for _ in range(50)]
    qs += ["w0", "w0 AND w1", "w49 OR w0", "w3 OR w4 OR w5 OR w6 OR w7", "w1 AND NOT w0", "w2 OR " + NO_MATCH,
           NO_MATCH, " OR ".join(vocab[:20])]
    return t, d, Truth(O.Index(t, d), tf_of_docs(docs)), qs


@pytest.mark.parametrize("own_slice", [False, True], ids=["all-slices", "own-slice"])
@pytest.mark.parametrize("world", [2, 3])
def test_emulated_ranks_explain_what_they_hold(nxs, shard_corpus, world, own_slice):
    """Every rank of an emulated world explains the responses it materialises -- an emulated rank holds its own
    block alone, so its own slice -- from its replica, with no collective; together they cover the batch.  A wide
    plan and a limit of 200 take the exact fix-up round first."""
    from nxsearch_amd import multi
    t, d, truth, qs = shard_corpus
    qs = qs + [" OR ".join("w%d" % i for i in range(33))]
    gidx = nxs.open_files(t, d)
    for limit in (10, 200):
        plain = gidx.search_batch(qs, limit=limit, fuzzymatch=False)
        covered = 0
        for rank in range(world):
            multi.emulate(gidx, rank, world)
            gidx.shard_local(own_slice)
            lo, hi = multi.shard_slice(len(qs), rank, world)
            got = gidx.search_batch(qs, limit=limit, fuzzymatch=False, explain=True)
            assert len(multi.emulated_block(gidx)) == multi.block_bytes(multi.shard_capacity(len(qs), world), limit)
            for i, (q, g) in enumerate(zip(qs, got)):
                if lo <= i < hi:
                    check(g, plain[i], truth, q, O.BM25, False, ("emulated", world, rank, limit))
                    covered += 1
                else:
                    assert isinstance(g, N.NxsError), (rank, i)         # another rank's slice: not held here
            # without the key an emulated rank hands out its block only, as before
            assert all(isinstance(g, N.NxsError) for g in gidx.search_batch(qs, limit=limit, fuzzymatch=False))
        assert covered == len(qs)
        multi.emulate(gidx, 0, 0)
        gidx.shard_local(False)
    gidx.close()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_doc_shards_explain_from_the_shard_that_holds_the_doc(nxs, shard_corpus, n_shards):
    t, d, truth, qs = shard_corpus
    shards = [nxs.open_shard(t, d, s_, n_shards) for s_ in range(n_shards)]
    for limit in (10, 300):
        for algo in ALGOS:
            plain = nxs.docshard_search_batch(shards, qs, limit=limit, algo=algo, fuzzymatch=False)
            got = nxs.docshard_search_batch(shards, qs, limit=limit, algo=algo, fuzzymatch=False, explain=True)
            for q, g, p in zip(qs, got, plain):
                check(g, p, truth, q, ALGOS[algo][0], False, ("doc shards", n_shards, limit, algo))
                # ... and the whole-index oracle's results
                w = truth.oidx.search(q, algo=ALGOS[algo][0], limit=limit, fuzzymatch=False)
                assert [x for x, _ in g] == [x for x, _ in w], (q, limit, algo)
    for s_ in shards:
        assert s_.explain_profile()["passes"] == 4
        s_.close()


def test_ranked_doc_shard_batch_refuses(nxs, shard_corpus):
    t, d, truth, qs = shard_corpus
    sh = nxs.open_shard(t, d, 0, 1)
    sh.shard(0, 1, nxs.shard_unique_id())
    nxs.docshard_attach(sh)
    with pytest.raises(N.NxsError) as e:
        nxs.docshard_search_batch_rank(sh, qs[:4], limit=10, fuzzymatch=False, explain=True)
    assert e.value.code == 3 and e.value.msg == "explain is not available on a ranked doc-shard batch"
    got = nxs.docshard_search_batch_rank(sh, qs[:4], limit=10, fuzzymatch=False)
    for q, g in zip(qs[:4], got):
        assert [x for x, _ in g] == [x for x, _ in truth.oidx.search(q, limit=10, fuzzymatch=False)]
    # a communicator of one rank attached: the batch is this rank's, explained from its replica
    plain = sh.search_batch(qs, limit=10, fuzzymatch=False)
    for q, g, p in zip(qs, sh.search_batch(qs, limit=10, fuzzymatch=False, explain=True), plain):
        check(g, p, truth, q, O.BM25, False, "world 1")
    sh.close()


# ---- cost when not asked ------------------------------------------------------------------------------

def test_a_batch_that_does_not_ask_runs_no_pass(nxs, shard_corpus):
    t, d, truth, qs = shard_corpus
    gidx = nxs.open_files(t, d)
    gidx.search_batch(qs, limit=10, fuzzymatch=False)
    gidx.search_batch(qs, limit=1000, fuzzymatch=False, total=True)
    gidx.search(qs[0])
    assert gidx.explain_profile() == {"passes": 0, "ms": 0.0, "cells": 0, "present": 0, "chunks": 0}
    gidx.search_batch([NO_MATCH], limit=10, fuzzymatch=False, explain=True)         # asked, nothing to explain
    assert gidx.explain_profile()["passes"] == 0
    gidx.set_profiling(True)
    gidx.search_batch(qs, limit=10, fuzzymatch=False, explain=True)
    prof = gidx.explain_profile(reset=True)
    assert prof["passes"] == 1 and prof["chunks"] == 1 and prof["ms"] > 0 and 0 < prof["present"] <= prof["cells"], prof
    assert gidx.explain_profile()["passes"] == 0
    gidx.close()
