"""GPU tier (`-m gpu`) for prefix matching: Index.complete -> nxs_index_complete_batch -> nxsgpu_complete, and
`term*` leaves in searches ("prefixmatch").

Truth is computed in Python (complete_truth.Truth) from the corpus the test itself wrote: df = the number of
non-removed docs that hold the term, the match is term.startswith(p), the order df descending, term id
ascending.  Every prefix of every test is compared in full: terms (ids), distances, dfs, order, the list's
length and `matches`.  For searches the truth is the REWRITTEN query -- each `p*` replaced by the
parenthesised OR of the truth's expansions -- on the GPU and on the CPU oracle."""
import ctypes as C
import json
import random

import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from complete_truth import (big_corpus, big_prefixes, docs_of, random_words, rewrite, truth_of_docs,
                            truth_of_events)

pytestmark = pytest.mark.gpu

KS = (1, 5, 32)
ROUTES = pytest.mark.parametrize("route", [None, "host"], ids=["device", "host"])


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def make_index(nxs, tmp_path, name, term_dfs, dead=(), lowercase=False):
    docs, removed = docs_of(term_dfs, dead)
    t, d, term_ids = nxsfmt.write_index(str(tmp_path), name, docs, removed=removed)
    truth = truth_of_docs(docs, removed, term_ids)
    for term, df in term_dfs:
        assert truth.dfs[term_ids[term] - 1] == df
    for term in dead:
        assert truth.dfs[term_ids[term] - 1] == 0
    return nxs.open_files(t, d, lowercase=lowercase), truth


def check(gidx, truth, prefixes, k=None, ctx=None):
    """Index.complete against the truth, every prefix in full -> the lists"""
    got = gidx.complete(prefixes, limit=k)
    assert len(got) == len(prefixes)
    for p, g in zip(prefixes, got):
        want, m = truth.rank_terms(p, 5 if k is None else k)
        assert not isinstance(g, N.NxsError), (ctx, p, g)
        assert list(g) == want, (ctx, p, k)
        assert g.matches == m and g.dropped is False, (ctx, p, k, g.matches, m)
    return got


def shim(gidx, prefixes, k):
    """nxsgpu_complete itself -> [([(term id, df)], matches)]"""
    L = N.lib()
    n = len(prefixes)
    offs = [0]
    for p in prefixes:
        offs.append(offs[-1] + len(p))
    ids, df = (C.c_uint32 * (n * k))(), (C.c_uint32 * (n * k))()
    cnt, m = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    r = L.nxsgpu_complete(gidx.device, b"".join(prefixes) + b"\0" * 16, (C.c_uint32 * (n + 1))(*offs), n, k,
                          ids, df, cnt, m)
    assert r == 0, L.nxsgpu_last_error()
    return [([(ids[i * k + j], df[i * k + j]) for j in range(cnt[i])], m[i]) for i in range(n)]


def set_route(monkeypatch, gidx, route):
    """NXS_GPU_COMPLETE: None = the device pass, "host" = the host ranker for everything"""
    if route is None:
        monkeypatch.delenv("NXS_GPU_COMPLETE", raising=False)
    else:
        monkeypatch.setenv("NXS_GPU_COMPLETE", route)
    gidx.reconfigure()


@pytest.fixture(scope="module")
def big(nxs, tmp_path_factory):
    term_dfs, dead, words = big_corpus()
    gidx, truth = make_index(nxs, tmp_path_factory.mktemp("big"), "big", term_dfs, dead=dead)
    yield gidx, truth, big_prefixes(words), words
    gidx.close()


# ---- 1. random parity ----------------------------------------------------------------------

@ROUTES
def test_random_parity(big, monkeypatch, route):
    """306 prefixes and a batch of one, every k, on the device pass and on the host ranker; the shim's term
    ids against the truth's."""
    gidx, truth, prefixes, words = big
    set_route(monkeypatch, gidx, route)
    gidx.complete_profile(reset=True)
    try:
        for k in KS:
            check(gidx, truth, prefixes, k, route)
            check(gidx, truth, prefixes[5:6], k, route)
        assert check(gidx, truth, prefixes[:7]) == check(gidx, truth, prefixes[:7], 5)      # the default
        for (rows, m), p in zip(shim(gidx, prefixes, 5), prefixes):
            assert (rows, m) == truth.rank(p, 5), p
        # a whole word completes to itself, a dead word does not, the over-long prefix matches nothing
        whole = next(w for w in words[:1900] if len(w) >= 8)
        assert (whole, 0) in [(t, d) for t, d, _ in gidx.complete([whole], limit=32)[0]]
        assert words[1950] not in [t for t, _, _ in gidx.complete([words[1950]], limit=32)[0]]
        last = gidx.complete([prefixes[-1]])[0]
        assert last == [] and last.matches == 0
        prof = gidx.complete_profile()
        assert prof["host_prefixes"] == (0 if route is None else 3 * 307 + 14 + 306 + 3)
        assert prof["builds"] <= 1 and prof["entries"] in (0, 1940)
    finally:
        set_route(monkeypatch, gidx, None)


# ---- 2. range edges ------------------------------------------------------------------------

@ROUTES
def test_range_edges(nxs, tmp_path, monkeypatch, route):
    """Prefixes below every term, above every term, between two terms, equal to the first and the last term of
    the order, and one that ends in 0xFF with extensions present; a dictionary of one term."""
    terms = [b"a\xff", b"a\xffz", b"b", b"bd", b"bdx", b"df", b"dz"]
    gidx, truth = make_index(nxs, tmp_path, "edges", [(w, 1 + i % 3) for i, w in enumerate(terms)])
    set_route(monkeypatch, gidx, route)
    try:
        prefixes = [b"A", b"e", b"\xff", b"c", b"be", b"a\xff", b"dz", b"a", b"a\xffz", b"a\xffzz", b"b", b"bd", b"d",
                    b"a\xfe", b"dzz"]
        for k in KS:
            got = check(gidx, truth, prefixes, k, route)
            assert [g.matches for g in got] == [0, 0, 0, 0, 0, 2, 1, 2, 1, 0, 3, 2, 2, 0, 0]
        g = gidx.complete([b"a\xff"], limit=5)[0]
        assert g == [(b"a\xffz", 1, 2), (b"a\xff", 0, 1)] and g.matches == 2
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()
    solo, truth = make_index(nxs, tmp_path, "solo", [(b"solo", 2)])
    set_route(monkeypatch, solo, route)
    try:
        got = check(solo, truth, [b"s", b"solo", b"solox", b"a", b"z", b"sol"], 5, route)
        assert [g.matches for g in got] == [1, 1, 0, 0, 0, 1] and got[1] == [(b"solo", 0, 2)]
    finally:
        set_route(monkeypatch, solo, None)
        solo.close()


# ---- 3. chunk boundaries of the sort -------------------------------------------------------

@ROUTES
def test_sort_chunk_boundaries(nxs, tmp_path, monkeypatch, route):
    """Terms that agree on their first 7 / 8 / 9 / 15 / 16 / 17 bytes and differ only after, a 70-byte and a
    200-byte term with a common 66-byte prefix: the order is checked through `matches` -- every prefix of
    every term counts exactly the terms Python counts."""
    base = bytes(random.Random(5).choice(b"abcdef") for _ in range(200))
    terms = [base[:n] + s for n in (7, 8, 9, 15, 16, 17) for s in (b"x", b"y")] + [base[:66] + b"pqrs", base]
    terms += [b"ab", b"fe"]
    assert len(terms[12]) == 70 and len(terms[13]) == 200
    gidx, truth = make_index(nxs, tmp_path, "chunks", [(w, 1 + i % 4) for i, w in enumerate(terms)])
    set_route(monkeypatch, gidx, route)
    try:
        prefixes = sorted({t[:n] for t in terms for n in range(1, len(t) + 1)})
        for n in (7, 8, 9, 16, 17, 66):
            assert base[:n] in prefixes
        got = check(gidx, truth, prefixes, 32, route)
        assert got[prefixes.index(base[:7])].matches == 14 and got[prefixes.index(base[:17])].matches == 4
        assert got[prefixes.index(base[:66])].matches == 2 and got[prefixes.index(base[:67])].matches == 1
        check(gidx, truth, [base[:7], base[:8], base[:9], base[:16], base[:17], base[:66]], 1, route)
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 4. selection sizes --------------------------------------------------------------------

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513)


@ROUTES
def test_selection_sizes(nxs, tmp_path, monkeypatch, route):
    """Ranges of 0, 1, 63, 64, 65, 255, 256, 257 and 513 eligible terms (255 / 256: where a thread's first entry
    ends and its stride begins in the 256-thread selection; 513: threads stride twice): with equal df (`e<n>_`:
    the term id decides) and with df strictly increasing with the term id (`i<n>_`: the last entries win)."""
    term_dfs = []
    for n in SIZES:
        term_dfs += [(b"e%d_%03d" % (n, j), 3) for j in range(n)]
    for n in SIZES:
        term_dfs += [(b"i%d_%03d" % (n, j), j + 1) for j in range(n)]
    gidx, truth = make_index(nxs, tmp_path, "sizes", term_dfs)
    set_route(monkeypatch, gidx, route)
    try:
        prefixes = [b"e%d_" % n for n in SIZES] + [b"i%d_" % n for n in SIZES] + [b"e", b"i", b"e6", b"i25"]
        for k in KS:
            got = check(gidx, truth, prefixes, k, route)
            ns = len(SIZES)
            assert [g.matches for g in got[:2 * ns]] == list(SIZES) * 2
            for n, g in zip(SIZES, got[:ns]):
                assert [t for t, _, _ in g] == [b"e%d_%03d" % (n, j) for j in range(min(k, n))]
            for n, g in zip(SIZES, got[ns:2 * ns]):
                assert [df for _, _, df in g] == list(range(n, n - min(k, n), -1))
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


@ROUTES
def test_one_byte_prefix_over_20000_terms(nxs, tmp_path, monkeypatch, route):
    """A one-byte prefix over a 20 000-term dictionary: ranges of ~3300 entries, every thread of the
    selection strides over the range; `matches` and the 32 best are exact."""
    rng = random.Random(20000)
    words = random_words(rng, 20000, lo=3, hi=9)
    gidx, truth = make_index(nxs, tmp_path, "wide", [(w, rng.choice([1, 1, 1, 2, 2, 3])) for w in words])
    set_route(monkeypatch, gidx, route)
    try:
        prefixes = [bytes([c]) for c in b"abcdef"] + [b"ab", b"fe", b"g"]
        got = check(gidx, truth, prefixes, 32, route)
        assert sum(g.matches for g in got[:6]) == 20000 and min(g.matches for g in got[:6]) > 3000
        check(gidx, truth, prefixes, 1, route)
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 5. liveness and refresh ---------------------------------------------------------------

def test_liveness_and_refresh(nxs, tmp_path):
    ev = [("add", 10, ["apple", "maple", "zebra"]), ("add", 20, ["apple", "apply"]), ("add", 30, ["ample", "apple"]),
          ("add", 40, ["apply", "zebra"]), ("add", 50, ["ample"]), ("add", 60, ["apricot"]), ("rm", 60)]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 262144)
    open(d, "wb").write(dimg + b"\0" * 262144)
    gidx = nxs.open_files(t, d)

    def publish():
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        nxsfmt.publish_in_place(t, d, timg, dimg)
        return truth_of_events(ev)
    prefixes = [b"ap", b"a", b"z", b"apr"]
    assert gidx.complete_profile()["builds"] == 0               # never asked: nothing built
    before = check(gidx, truth_of_events(ev), prefixes, 5, "snapshot 0")
    # the term whose only doc is removed is neither listed nor counted
    assert before[0] == [(b"apple", 3, 3), (b"apply", 3, 2)] and before[0].matches == 2
    assert before[3] == [] and before[3].matches == 0
    assert gidx.complete_profile()["builds"] == 1
    check(gidx, truth_of_events(ev), prefixes, 32, "again")
    check(gidx, truth_of_events(ev), prefixes[:1], 1, "again")
    assert gidx.complete_profile()["builds"] == 1               # repeated calls: no rebuild
    ev += [("rm", 20), ("rm", 40)]                              # every doc of "apply"
    after = check(gidx, publish(), prefixes, 5, "removal")
    assert after[0] == [(b"apple", 3, 2)] and after[0].matches == 1
    assert gidx.complete_profile()["builds"] == 2
    ev.append(("add", 70, ["applq", "zebra", "apricot"]))      # a new term, and a dead one comes back
    newer = check(gidx, publish(), prefixes, 5, "append")
    assert newer[0] == [(b"apple", 3, 2), (b"apricot", 5, 1), (b"applq", 3, 1)] and newer[0].matches == 3
    assert newer[3] == [(b"apricot", 4, 1)]
    check(gidx, truth_of_events(ev), prefixes, 5, "again")
    prof = gidx.complete_profile()
    assert prof["builds"] == 3 and prof["entries"] == 6
    gidx.close()


# ---- 6. concurrency and refusals -----------------------------------------------------------

def test_beside_batches_in_flight(big):
    gidx, truth, prefixes, words = big
    rng = random.Random(10)
    toks = [w.decode() for w in words[:400] if len(w) >= 3]
    qa = ["%s OR %sx" % (rng.choice(toks), rng.choice(toks)) for _ in range(96)]         # misses: a fuzzy pass
    qb = ["%s AND %s" % (rng.choice(toks), rng.choice(toks)) for _ in range(80)]
    alone_a, alone_b = gidx.search_batch(qa, limit=10), gidx.search_batch(qb, limit=10)
    alone = check(gidx, truth, prefixes, 5, "alone")
    gidx.search_batch_begin(qa, limit=10)
    assert check(gidx, truth, prefixes, 5, "one in flight") == alone
    assert gidx.search_batch_end() == alone_a
    gidx.search_batch_begin(qa, limit=10)
    gidx.search_batch_begin(qb, limit=10)
    assert check(gidx, truth, prefixes[:40], 32, "two in flight") == check(gidx, truth, prefixes[:40], 32)
    assert gidx.search_batch_end() == alone_a
    assert check(gidx, truth, prefixes, 5, "one left") == alone
    assert gidx.search_batch_end() == alone_b


def complete_one(gidx, prefix, limit=None, as_json=False):
    """nxs_index_complete()"""
    L = N.lib()
    p = None
    if limit is not None:
        p = L.nxs_params_create()
        L.nxs_params_set_uint(p, b"complete_limit", limit)
    pb = N._b(prefix)
    try:
        sg = L.nxs_index_complete(gidx._h, p, pb, len(pb))
    finally:
        if p:
            L.nxs_params_release(p)
    if not sg:
        gidx.nxs._raise()
    return N._drain_sugg(sg, as_json)


def test_api_surface_and_refusals(nxs, tmp_path):
    term_dfs = [(b"hello", 2), (b"hallo", 3), (b"help", 1), (b"world", 1), (b"he", 1)]
    docs, _ = docs_of(term_dfs)
    t, d, term_ids = nxsfmt.write_index(str(tmp_path), "api", docs)
    truth = truth_of_docs(docs, (), term_ids)
    gidx = nxs.open_files(t, d, lowercase=True)
    want = check(gidx, truth, [b"he"], 5)[0]
    assert want == [(b"hello", 3, 2), (b"help", 2, 1), (b"he", 0, 1)] and want.matches == 3
    got = gidx.complete(["HE", "he", "He", "he"])
    assert got == [want] * 4                                          # lowercased; duplicates: equal lists
    assert complete_one(gidx, "HE") == want
    sg = N.lib().nxs_index_complete(gidx._h, None, b"HExyz", 2)       # the length is the caller's
    assert sg and N._drain_sugg(sg) == want
    one = complete_one(gidx, "H", limit=2)
    assert (list(one), one.matches) == truth.rank_terms(b"h", 2) and one.matches == 4
    doc = json.loads(complete_one(gidx, "HE", as_json=True))
    assert list(doc) == ["prefix", "completions", "matches"] and doc["prefix"] == "he" and doc["matches"] == 3
    assert [(s["term"].encode(), s["df"]) for s in doc["completions"]] == [(t_, df) for t_, _, df in want]
    assert gidx.complete(["HE"], json=True) == [complete_one(gidx, "he", as_json=True)]
    assert gidx.complete([]) == []
    # parameters out of range fail the call and name the key; an empty prefix is invalid
    for lim in (0, 33):
        with pytest.raises(N.NxsError) as e:
            gidx.complete(["he"], limit=lim)
        assert e.value.code == 3 and "complete_limit" in e.value.msg
        with pytest.raises(N.NxsError) as e:
            gidx.search("he*", prefixmatch=True, prefix_limit=lim)
        assert e.value.code == 3 and "prefix_limit" in e.value.msg
        with pytest.raises(N.NxsError) as e:
            gidx.search_batch_begin(["he*"], prefixmatch=True, prefix_limit=lim)
        assert e.value.code == 3 and "prefix_limit" in e.value.msg
    with pytest.raises(N.NxsError) as e:
        complete_one(gidx, "")
    assert e.value.code == 3 and "empty prefix" in e.value.msg
    got = gidx.complete(["he", "", "h"])
    assert isinstance(got[1], N.NxsError) and got[1].code == 3 and got[0] == want and got[2].matches == 4
    gidx.close()


def test_shards_and_communicators(nxs, tmp_path):
    term_dfs = [(b"hello", 2), (b"hallo", 3), (b"help", 1), (b"world", 1), (b"he", 1)]
    docs, _ = docs_of(term_dfs)
    t, d, term_ids = nxsfmt.write_index(str(tmp_path), "sh", docs)
    truth = truth_of_docs(docs, (), term_ids)
    # a doc shard refuses the call and a batch with a prefix leaf; without one it searches as ever
    sh = nxs.open_shard(t, d, 0, 1)
    with pytest.raises(N.NxsError) as e:
        sh.complete(["he"])
    assert e.value.code == 3 and e.value.msg == "complete is not available on a doc shard"
    with pytest.raises(N.NxsError) as e:
        nxs.docshard_search_batch([sh], ["hello", "he* AND world"], limit=5, prefixmatch=True)
    assert e.value.code == 3 and e.value.msg == "prefixmatch is not available on a doc shard"
    plain = nxs.docshard_search_batch([sh], ["hello", "world"], limit=5)
    assert nxs.docshard_search_batch([sh], ["hello", "world"], limit=5, prefixmatch=True) == plain and plain[0]
    sh.close()
    # a world-1 communicator answers, with a batch in flight too
    gidx = nxs.open_files(t, d)
    gidx.shard(0, 1, nxs.shard_unique_id())
    check(gidx, truth, [b"he", b"hal"], 5, "world 1")
    gidx.search_batch_begin(["hello OR helo"], limit=5)
    check(gidx, truth, [b"he", b"w"], 5, "world 1, a batch in flight")
    assert len(gidx.search_batch_end()) == 1
    assert gidx.search("he*", prefixmatch=True, fuzzymatch=False) == gidx.search("hello OR help OR he", fuzzymatch=False)
    gidx.shard(0, 1, None)
    check(gidx, truth, [b"he"], 5, "detached")
    gidx.close()


# ---- 7. queries ----------------------------------------------------------------------------

ALGOS = ((O.BM25, "BM25"), (O.TF_IDF, "TF-IDF"))


@pytest.fixture(scope="module")
def qcorpus(nxs, tmp_path_factory):
    """600 docs of 6-24 words out of a 400-word a-f vocabulary (lengths 2-6, Zipf-ish): lowercase on, no
    stemmer; the GPU index, the oracle's and the truth."""
    rng = random.Random(777)
    vocab = random_words(rng, 400, lo=2, hi=6)
    weights = [1.0 / (1 + i) ** 0.7 for i in range(len(vocab))]
    docs, did = [], 0
    for _ in range(600):
        did += rng.randint(1, 50)
        docs.append((did, rng.choices(vocab, weights, k=rng.randint(6, 24))))
    removed = [docs[i][0] for i in (3, 77, 300)]
    t, d, term_ids = nxsfmt.write_index(str(tmp_path_factory.mktemp("q")), "q", docs, removed=removed)
    truth = truth_of_docs(docs, set(removed), term_ids)
    gidx = nxs.open_files(t, d, lowercase=True)
    oidx = O.Index(t, d, lowercase=True)
    yield gidx, oidx, truth, [w.decode() for w in vocab]
    gidx.close()
    oidx.close()


def same(got, want, ctx):
    """doc ids and order exact, scores within 1e-5 relative"""
    assert [dd for dd, _ in got] == [dd for dd, _ in want], ctx
    for (_, a), (_, b) in zip(got, want):
        assert abs(a - b) <= 1e-5 * max(abs(a), abs(b)), ctx


def query_shapes(truth, vocab):
    """-> [(Q, prefix_limit, expect hits)]"""
    n2 = lambda p: len(truth.eligible(p.encode()))
    two = sorted({w[:2] for w in vocab}, key=lambda p: (-n2(p), p))
    p9 = next(p for p in two if n2(p) >= 9)                     # at least 9 expansions
    pa, pb = [p for p in two if 3 <= n2(p) <= 8][:2]
    lit = truth.expansions(pa.encode(), 8)[1].decode()          # an expansion that is also a literal token
    c, e = vocab[0], vocab[1]                                   # the two most frequent words
    assert n2("a") > 32 and n2("b") > 32 and n2("zz") == 0
    return [
        ("%s*" % pa, 8, True),
        ("%s* AND %s" % (pa, c), 8, True),
        ("%s AND NOT %s*" % (c, pa), 8, True),
        ("(%s* OR %s*) AND %s" % (pa, pb, e), 8, True),
        ("zz*", 8, False),
        ("zz* AND %s" % c, 8, False),
        ("zz* OR %s" % c, 8, True),
        ("%s OR %s* OR %s" % (lit, pa, c), 8, True),
        ("%s AND (%s* OR %s)" % (lit, pa, e), 8, True),
        ("%s*" % p9, 1, True),
        ("%s*" % p9, 8, True),
        ("%s*" % p9, 32, True),
        ("%s* %s" % (p9, c), 8, True),                          # 9 live tokens: no truth table
        ("%s* AND NOT %s" % (p9, c), 9, True),
        ("a* OR b* OR %s" % c, 32, True),                       # 65 tokens: the wide plan
        ("(a* AND b*) AND NOT %s*" % p9, 32, True),
        ("%s* AND %s*" % (pa.upper(), pb), 8, None),            # the prefix is lowercased
        ('"%s*" OR %s' % (pa, c), 8, True),                     # a quoted star is an ordinary leaf
        ("* OR %s*" % pa, 8, True),                             # so is a lone one
    ]


def test_prefix_leaves_in_queries(qcorpus):
    gidx, oidx, truth, vocab = qcorpus
    shapes = query_shapes(truth, vocab)
    n_docs = oidx.doc_count
    # on the CPU first: the oracle has hits wherever the test expects some (two empty lists prove nothing)
    for q, pl, hits in shapes:
        r = rewrite(q, truth, pl)
        if hits is not None:
            assert bool(oidx.search(r, limit=n_docs, fuzzymatch=False)) == hits, (q, r)
    for oalgo, algo in ALGOS:
        for q, pl, hits in shapes:
            r = rewrite(q, truth, pl)
            for limit in (10, 1000):
                ctx = (q, r, pl, algo, limit)
                got = gidx.search(q, limit=limit, algo=algo, fuzzymatch=False, prefixmatch=True, prefix_limit=pl)
                same(got, gidx.search(r, limit=limit, algo=algo, fuzzymatch=False), ctx)
                same(got, oidx.search(r, algo=oalgo, limit=limit, fuzzymatch=False), ctx)
            # total: the oracle's count with the limit lifted
            got = gidx.search(q, limit=10, algo=algo, fuzzymatch=False, prefixmatch=True, prefix_limit=pl, total=True)
            want = len(oidx.search(r, algo=oalgo, limit=n_docs, fuzzymatch=False))
            assert got.total == want, (q, r, algo, got.total, want)
    # the default prefix_limit is 8
    q = shapes[10][0]
    assert gidx.search(q, prefixmatch=True, fuzzymatch=False) == gidx.search(q, prefixmatch=True, prefix_limit=8, fuzzymatch=False)
    assert gidx.search(q, prefixmatch=True, fuzzymatch=False) != gidx.search(q, prefixmatch=True, prefix_limit=32, fuzzymatch=False)


def test_other_leaves_are_still_fuzzy_matched(qcorpus):
    gidx, oidx, truth, vocab = qcorpus
    long_w = next(w for w in vocab if len(w) == 6)
    typo = long_w[:3] + "z" + long_w[4:]
    assert truth.rank(typo.encode(), 1)[1] == 0
    pa = query_shapes(truth, vocab)[0][0]
    for q in ("%s AND %s" % (pa, typo), "%s OR %s" % (typo, pa), "zz* OR %s" % typo):
        r = rewrite(q, truth, 8)
        assert oidx.search(r, limit=1000), (q, r)
        got = gidx.search(q, limit=1000, prefixmatch=True)
        same(got, gidx.search(r, limit=1000), (q, r))
        same(got, oidx.search(r, limit=1000), (q, r))
    # the prefix itself is never fuzzy-matched: two edits away from words, no term begins with it
    far = long_w[:4] + "zz"
    assert gidx.search(far[:5], limit=10) and gidx.search("%s*" % far[:5], limit=10, prefixmatch=True) == []


def test_flag_absent_nothing_changes(qcorpus):
    """Without prefixmatch (absent or false) `ab*` is the verbatim token it always was -- and the plan cache
    keeps the two readings of one string apart."""
    gidx, oidx, truth, vocab = qcorpus
    shapes = query_shapes(truth, vocab)
    for fuzzy in (False, True):
        for q, pl, _ in shapes[:9] + shapes[-3:]:
            want = oidx.search(q, limit=10, fuzzymatch=fuzzy)
            with_px = gidx.search(q, limit=10, fuzzymatch=fuzzy, prefixmatch=True, prefix_limit=pl)
            same(gidx.search(q, limit=10, fuzzymatch=fuzzy), want, (q, fuzzy))
            same(gidx.search(q, limit=10, fuzzymatch=fuzzy, prefixmatch=False), want, (q, fuzzy))
            same(gidx.search(q, limit=10, fuzzymatch=fuzzy, prefix_limit=3), want, (q, fuzzy))
            assert gidx.search(q, limit=10, fuzzymatch=fuzzy, prefixmatch=True, prefix_limit=pl) == with_px
    q = shapes[0][0]
    assert gidx.search(q, limit=10, fuzzymatch=False) == [] and gidx.search(q, limit=10, fuzzymatch=False, prefixmatch=True)


def test_batches_with_prefix_leaves(qcorpus):
    """A 64-query batch mixing prefixed and plain queries, blocking and through _begin/_end with two in
    flight; plan_batch compiles the rewritten query's plan."""
    gidx, oidx, truth, vocab = qcorpus
    rng = random.Random(64)
    shapes = [s for s in query_shapes(truth, vocab) if s[1] == 8]
    qs = []
    for i in range(64):
        if i % 3 == 0:
            qs.append("%s AND %s" % (rng.choice(vocab[:40]), rng.choice(vocab[:40])))
        elif i % 3 == 1:
            qs.append(rng.choice(shapes)[0])
        else:
            qs.append("%s* OR %s" % (rng.choice(vocab)[:2], rng.choice(vocab[:40])))
    rs = [rewrite(q, truth, 8) for q in qs]
    assert sum(1 for r in rs if oidx.search(r, limit=10, fuzzymatch=False)) > 40
    want = [gidx.search(r, limit=10, fuzzymatch=False) for r in rs]
    for r, w in zip(rs, want):
        same(w, oidx.search(r, limit=10, fuzzymatch=False), r)
    assert gidx.search_batch(qs, limit=10, fuzzymatch=False, prefixmatch=True) == want
    plain = gidx.search_batch(qs, limit=10, fuzzymatch=False)
    assert plain != want
    gidx.search_batch_begin(qs, limit=10, fuzzymatch=False, prefixmatch=True)
    gidx.search_batch_begin(qs, limit=10, fuzzymatch=False)
    gidx.search_batch_begin(qs[::-1], limit=10, fuzzymatch=False, prefixmatch=True, prefix_limit=8)
    assert gidx.search_batch_end() == want
    assert gidx.search_batch_end() == plain
    assert gidx.search_batch_end() == want[::-1]
    # with fuzzy matching on: the misses' pass may still be pending when the next batch begins
    typo = [q + " OR " + vocab[5][:-1] + "z" for q in qs[:32]]
    rs2 = [rewrite(q, truth, 8) for q in typo]
    want2 = gidx.search_batch(rs2, limit=10)
    gidx.search_batch_begin(typo, limit=10, prefixmatch=True)
    gidx.search_batch_begin(qs, limit=10, fuzzymatch=False, prefixmatch=True)
    assert gidx.search_batch_end() == want2
    assert gidx.search_batch_end() == want
    # plans
    sel = [i for i, r in enumerate(rs) if "(" in r][:8]
    got, errs = gidx.plan_batch([qs[i] for i in sel], fuzzymatch=False, prefixmatch=True)
    ref, errs_r = gidx.plan_batch([rs[i] for i in sel], fuzzymatch=False)
    assert errs == errs_r == [0] * len(sel)
    assert bytes(got)[:C.sizeof(N.GpuQuery) * len(sel)] == bytes(ref)[:C.sizeof(N.GpuQuery) * len(sel)]
