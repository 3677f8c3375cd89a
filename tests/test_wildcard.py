"""GPU tier (`-m gpu`) for wildcard matching: Index.wildcard -> nxs_index_wildcard_batch -> nxsgpu_wildcard, and
`*` / `?` leaves in searches ("wildcardmatch").

Truth is computed in Python (wild_truth.WildTruth) from the corpus the test itself wrote: df = the number of
non-removed docs that hold the term, the match a regex built from the pattern, the order df descending, term id
ascending.  Every pattern of every test is compared in full: terms (ids), distances, dfs, order, the list's
length and `matches`.  For searches the truth is the REWRITTEN query on the GPU and on the CPU oracle.  Every
test runs on both routes: the device pass and NXS_GPU_WILDCARD=host."""
import contextlib
import ctypes as C
import json
import random
import struct

import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from complete_truth import big_corpus, docs_of, random_words, truth_of_events as px_truth_of_events
from wild_truth import WildTruth, big_patterns, rewrite, truth_of_docs

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
    return nxs.open_files(t, d, lowercase=lowercase), truth


def check(gidx, truth, patterns, k=None, ctx=None):
    """Index.wildcard against the truth, every pattern in full -> the lists"""
    got = gidx.wildcard(patterns, limit=k)
    assert len(got) == len(patterns)
    for p, g in zip(patterns, got):
        want, m = truth.rank_terms(p, 5 if k is None else k)
        assert not isinstance(g, N.NxsError), (ctx, p, g)
        assert list(g) == want, (ctx, p, k)
        assert g.matches == m and g.dropped is False, (ctx, p, k, g.matches, m)
    return got


def shim(gidx, patterns, k):
    """nxsgpu_wildcard itself -> [([(term id, df)], matches)]"""
    L = N.lib()
    n = len(patterns)
    offs = [0]
    for p in patterns:
        offs.append(offs[-1] + len(p))
    ids, df = (C.c_uint32 * (n * k))(), (C.c_uint32 * (n * k))()
    cnt, m = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    r = L.nxsgpu_wildcard(gidx.device, b"".join(patterns) + b"\0" * 16, (C.c_uint32 * (n + 1))(*offs), n, k,
                          ids, df, cnt, m)
    assert r == 0, L.nxsgpu_last_error()
    return [([(ids[i * k + j], df[i * k + j]) for j in range(cnt[i])], m[i]) for i in range(n)]


def set_route(monkeypatch, gidx, route, parts=None):
    """NXS_GPU_WILDCARD: None = the device pass, "host" = the host ranker; NXS_GPU_WILD_PARTS"""
    for key, v in (("NXS_GPU_WILDCARD", route), ("NXS_GPU_WILD_PARTS", parts)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(v))
    gidx.reconfigure()


@contextlib.contextmanager
def routed(monkeypatch, gidx, route):
    """the body's wildcard leaves and calls take `route`, and only that route: the profile's counters say so"""
    set_route(monkeypatch, gidx, route)
    gidx.wildcard_profile(reset=True)
    try:
        yield
        prof = gidx.wildcard_profile()
        took, other = ("device_patterns", "host_patterns") if route is None else ("host_patterns", "device_patterns")
        assert prof[took] > 0 and prof[other] == 0, (route, prof)
    finally:
        set_route(monkeypatch, gidx, None)


@pytest.fixture(scope="module")
def big(nxs, tmp_path_factory):
    term_dfs, dead, words = big_corpus()
    gidx, truth = make_index(nxs, tmp_path_factory.mktemp("big"), "big", term_dfs, dead=dead)
    yield gidx, truth, big_patterns(words), words
    gidx.close()


# ---- 1. random parity ----------------------------------------------------------------------

@ROUTES
@pytest.mark.parametrize("parts", [1, 3, 64])
def test_random_parity(big, monkeypatch, route, parts):
    """300 patterns and a batch of one on the 1940-live-term index, every k: parts = 1 (one workgroup walks all
    8 tiles: the running top-k), 3 (uneven parts), 64 (a tile per workgroup: the merge carries everything)."""
    gidx, truth, patterns, words = big
    set_route(monkeypatch, gidx, route, parts)
    gidx.wildcard_profile(reset=True)
    try:
        for k in KS:
            check(gidx, truth, patterns, k, (route, parts))
            check(gidx, truth, patterns[2:3], k, (route, parts))
            for (rows, m), p in zip(shim(gidx, patterns, k), patterns):
                assert (rows, m) == truth.rank(p, k), (p, k, parts)
        assert check(gidx, truth, patterns[:7]) == check(gidx, truth, patterns[:7], 5)      # the default
        prof = gidx.wildcard_profile()
        n = 3 * (300 + 1 + 300) + 14
        assert (prof["host_patterns"], prof["device_patterns"]) == ((0, n) if route is None else (n, 0))
        assert prof["entries"] == 1940
    finally:
        set_route(monkeypatch, gidx, None)


# ---- 2. edges of the selection -------------------------------------------------------------

def edge_terms(k, fill):
    """Patterns with exactly c in (0, 1, k - 1, k, k + 1) matches, laid out three ways among the fillers (which
    hold no digit, x, y, w or ~): `x` = all in one tile (adjacent in the byte order, right behind the filler at
    position 522: every count's group lies in the third tile), `y` = one per 256-entry tile (match
    j extends the filler at position 256 j + 128 of the order), `w` = all at the very end of the order, in its
    last, partial tile."""
    counts = sorted({0, 1, k - 1, k, k + 1})
    order = sorted(w for w, _ in fill)
    terms = []
    for c in counts:
        terms += [(order[522] + b"%02d%02dx%02dz" % (c, j, c), 1 + j % 3) for j in range(c)]
        terms += [(order[256 * j + 128] + b"y%02dz" % c, 2) for j in range(c)]                # equal df
        terms += [(b"~~%02d%02dw%02dz" % (c, j, c), 1 + j % 2) for j in range(c)]
    return counts, terms


@ROUTES
@pytest.mark.parametrize("k", [1, 5, 32])
def test_selection_edges(nxs, tmp_path, monkeypatch, route, k):
    rng = random.Random(k)
    fill = [(w, rng.choice([1, 2, 3])) for w in random_words(rng, 9000, alphabet="bcdefghijkl", lo=3, hi=7)]
    counts, special = edge_terms(k, fill)
    gidx, truth = make_index(nxs, tmp_path, "edges%d" % k, fill + special)
    order = sorted(truth.terms)
    spread = [order.index(t) // 256 for t, _ in special if t.endswith(b"y%02dz" % (k + 1))]
    assert len(set(spread)) == k + 1                                # one per tile
    for c in counts[1:]:                                            # all in one tile
        group = [order.index(t) for t, _ in special if t.endswith(b"x%02dz" % c)]
        assert len(group) == c and max(group) - min(group) == c - 1 and min(group) // 256 == max(group) // 256, c
    assert len(order) % 256 > 40 and len(order) // 256 == order.index(b"~~%02d00w%02dz" % (k + 1, k + 1)) // 256
    try:
        for parts in (1, 3, 64):
            set_route(monkeypatch, gidx, route, parts)
            pats = []
            for c in counts:
                pats += [b"*x%02dz" % c, b"*y%02dz" % c, b"*w%02dz" % c, b"~~*w%02dz" % c, b"?*y%02dz" % c]
            got = check(gidx, truth, pats, k, (route, parts))
            assert [g.matches for g in got] == [c for c in counts for _ in range(5)]
            # all matches with equal df: the term id decides
            for c, g in zip(counts, got[1::5]):
                ids = [truth.terms.index(t) for t, _, _ in g]
                assert ids == sorted(ids) and len(ids) == min(k, c)
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


@ROUTES
@pytest.mark.parametrize("n_terms", [1, 255, 256, 257])
def test_live_term_counts_at_the_tile(nxs, tmp_path, monkeypatch, route, n_terms):
    terms = [(b"t%03dq" % j, 1 + (j * 7) % 5) for j in range(n_terms)]
    gidx, truth = make_index(nxs, tmp_path, "n%d" % n_terms, terms, dead=[b"t999q", b"zzq"])
    set_route(monkeypatch, gidx, route)
    try:
        for k in KS:
            got = check(gidx, truth, [b"*q", b"t*q", b"t??0q", b"?00?q", b"*%03dq" % (n_terms - 1), b"*9q", b"*zq"], k, route)
            assert got[0].matches == got[1].matches == n_terms and got[4].matches == 1 and got[6].matches == 0
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 3. range edges ------------------------------------------------------------------------

@ROUTES
def test_range_edges(nxs, tmp_path, monkeypatch, route):
    terms = [b"a\xff", b"a\xffz", b"a\xffyz", b"b", b"bd", b"bdx", b"bxd", b"df", b"dz", b"dzz"]
    gidx, truth = make_index(nxs, tmp_path, "redges", [(w, 1 + i % 3) for i, w in enumerate(terms)])
    set_route(monkeypatch, gidx, route)
    try:
        pats = [b"c*d", b"A*z", b"e?", b"a\xff*", b"a\xff*z", b"a\xff?", b"dzz*", b"dzz?", b"dz*z", b"a\xff", b"b*d", b"b?d",
                b"b*", b"?d", b"b?", b"??x", b"?z*", b"\xff*a", b"d?", b"*\xff*", b"?\xff?", b"??z", b"b??"]
        for k in KS:
            got = check(gidx, truth, pats, k, route)
            assert [g.matches for g in got] == [0, 0, 0, 3, 2, 1, 1, 0, 1, 1, 2, 1, 4, 1, 1, 1, 2, 0, 2, 3, 1, 2, 2]
        # patterns of metacharacters alone are not served
        got = gidx.wildcard([b"??", b"?", b"???", b"*?"], limit=5)
        assert all(isinstance(g, N.NxsError) and g.code == 3 for g in got)
        # `head*` returns exactly what complete(head) returns
        for head in (b"a\xff", b"b", b"bd", b"d", b"dz", b"dzz", b"c", b"a"):
            w, c = gidx.wildcard([head + b"*"], limit=32)[0], gidx.complete([head], limit=32)[0]
            assert list(w) == list(c) and w.matches == c.matches, head
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 4. searches ---------------------------------------------------------------------------

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
    """doc ids, order and scores, bit for bit (the float's bits: the GPU's own run of the rewritten query and
    the CPU oracle's alike)"""
    assert [(d, struct.pack("<f", s)) for d, s in got] == [(d, struct.pack("<f", s)) for d, s in want], ctx


def query_shapes(truth, vocab):
    """-> [(Q, wildcard_terms)]"""
    c, e = vocab[0], vocab[1]
    w6 = next(w for w in vocab if len(w) == 6)
    assert len(truth.eligible(b"*a")) > 32 and len(truth.eligible(b"?z?z?")) == 0
    return [
        ("*%s" % w6[2:], 8), ("%s*%s" % (w6[:1], w6[-2:]), 8), ("%s?%s AND %s" % (w6[:2], w6[3:], c), 8),
        ("%s AND NOT *%s" % (c, w6[-2:]), 8), ("(*ab* OR ?c?) AND %s" % e, 8), ("?z?z?", 8), ("?z?z? AND %s" % c, 8),
        ("?z?z? OR %s" % c, 8), ("*a", 1), ("*a", 8), ("*a", 32), ("*a %s" % c, 8), ("*a OR *b OR %s" % c, 32),
        ("(a*a AND *b*) AND NOT ??", 32), ("%s*%s" % (w6[:1].upper(), w6[-2:]), 8), ('"*a" OR %s' % c, 8),
        ("* OR ?? OR a?", 8),
    ]


@ROUTES
def test_wildcard_leaves_in_queries(qcorpus, monkeypatch, route):
    gidx, oidx, truth, vocab = qcorpus
    with routed(monkeypatch, gidx, route):
        shapes = query_shapes(truth, vocab)
        n_docs = oidx.doc_count
        hits = 0
        for oalgo, algo in ALGOS:
            for q, wt in shapes:
                r = rewrite(q, truth, wt)
                for limit in (10, 1000):
                    ctx = (q, r, wt, algo, limit)
                    got = gidx.search(q, limit=limit, algo=algo, fuzzymatch=False, wildcardmatch=True, wildcard_terms=wt)
                    same(got, gidx.search(r, limit=limit, algo=algo, fuzzymatch=False), ctx)
                    same(got, oidx.search(r, algo=oalgo, limit=limit, fuzzymatch=False), ctx)
                    hits += bool(got)
                got = gidx.search(q, limit=10, algo=algo, fuzzymatch=False, wildcardmatch=True, wildcard_terms=wt,
                                  total=True, explain=True)
                ref = gidx.search(r, limit=10, algo=algo, fuzzymatch=False, total=True, explain=True)
                assert got.total == ref.total == len(oidx.search(r, algo=oalgo, limit=n_docs, fuzzymatch=False)), (q, r)
                assert list(got) == list(ref) and got.tokens == ref.tokens and got.explain == ref.explain, (q, r)
        assert hits > 40
        q = shapes[9][0]
        kw = dict(fuzzymatch=False, wildcardmatch=True)
        assert gidx.search(q, **kw) == gidx.search(q, wildcard_terms=8, **kw) != gidx.search(q, wildcard_terms=32, **kw)


@ROUTES
def test_mixing_with_prefix_and_fuzzy_leaves(qcorpus, monkeypatch, route):
    gidx, oidx, truth, vocab = qcorpus
    with routed(monkeypatch, gidx, route):
        long_w = next(w for w in vocab if len(w) == 6)
        typo = long_w[:3] + "z" + long_w[4:]
        for q in ("*a AND %s" % typo, "%s OR ?b*" % typo, "ab* OR *%s" % long_w[3:], "a* AND NOT (*b OR %s)" % typo):
            r = rewrite(q, truth, 8, prefixmatch=True, prefix_limit=4)
            assert oidx.search(r, limit=1000), (q, r)
            got = gidx.search(q, limit=1000, prefixmatch=True, prefix_limit=4, wildcardmatch=True)
            same(got, gidx.search(r, limit=1000), (q, r))
            same(got, oidx.search(r, limit=1000), (q, r))
        # the pattern itself is never fuzzy-matched
        far = long_w[:4] + "zz"
        assert gidx.search(far[:5], limit=10) and gidx.search("%s?" % far[:5], limit=10, wildcardmatch=True) == []


@ROUTES
def test_flag_absent_nothing_changes(qcorpus, monkeypatch, route):
    gidx, oidx, truth, vocab = qcorpus
    with routed(monkeypatch, gidx, route):
        for fuzzy in (False, True):
            for q, wt in query_shapes(truth, vocab) + [("mi*soft", 8), ("a?", 8)]:
                want = oidx.search(q, limit=10, fuzzymatch=fuzzy)
                with_wc = gidx.search(q, limit=10, fuzzymatch=fuzzy, wildcardmatch=True, wildcard_terms=wt)
                for kw in ({}, {"wildcardmatch": False}, {"wildcard_terms": 3}):
                    got = gidx.search(q, limit=10, fuzzymatch=fuzzy, **kw)
                    assert [d for d, _ in got] == [d for d, _ in want], (q, fuzzy, kw)
                assert gidx.search(q, limit=10, fuzzymatch=fuzzy, wildcardmatch=True, wildcard_terms=wt) == with_wc
        assert gidx.search("*a", limit=10, fuzzymatch=False) == [] and gidx.search("*a", limit=10, fuzzymatch=False, wildcardmatch=True)


@ROUTES
def test_batches_with_wildcard_leaves(qcorpus, monkeypatch, route):
    gidx, oidx, truth, vocab = qcorpus
    with routed(monkeypatch, gidx, route):
        rng = random.Random(64)
        shapes = [s[0] for s in query_shapes(truth, vocab) if s[1] == 8]
        qs = []
        for i in range(64):
            if i % 3 == 0:
                qs.append("%s AND %s" % (rng.choice(vocab[:40]), rng.choice(vocab[:40])))
            elif i % 3 == 1:
                qs.append(rng.choice(shapes))
            else:
                qs.append("*%s OR %s" % (rng.choice(vocab)[-2:], rng.choice(vocab[:40])))
        long_q = "a" * 255 + "*"
        qs[5] = long_q + " OR " + vocab[0]                     # fails its own query only
        rs = [rewrite(q, truth, 8) for q in qs]
        kw = dict(limit=10, fuzzymatch=False)
        want = [gidx.search(r, **kw) if i != 5 else None for i, r in enumerate(rs)]
        got = gidx.search_batch(qs, wildcardmatch=True, **kw)
        assert isinstance(got[5], N.NxsError) and got[5].code == 3
        assert [g for i, g in enumerate(got) if i != 5] == [w for i, w in enumerate(want) if i != 5]
        with pytest.raises(N.NxsError) as e:
            gidx.search(long_q, wildcardmatch=True)
        assert e.value.code == 3 and "wildcard pattern too long" in e.value.msg
        ok = [q for i, q in enumerate(qs) if i != 5]
        want = [w for i, w in enumerate(want) if i != 5]
        assert sum(1 for w in want if w) > 40
        plain = gidx.search_batch(ok, **kw)
        assert plain != want
        gidx.search_batch_begin(ok, wildcardmatch=True, **kw)
        gidx.search_batch_begin(ok, **kw)
        gidx.search_batch_begin(ok[::-1], wildcardmatch=True, wildcard_terms=8, **kw)
        assert gidx.search_batch_end() == want
        assert gidx.search_batch_end() == plain
        assert gidx.search_batch_end() == want[::-1]
        # the call itself beside batches in flight
        alone = check(gidx, truth, [b"*a", b"a?", b"?b*"], 5)
        gidx.search_batch_begin(ok, wildcardmatch=True, **kw)
        assert check(gidx, truth, [b"*a", b"a?", b"?b*"], 5, "in flight") == alone
        assert gidx.search_batch_end() == want
        # plans
        sel = [i for i, r in enumerate(rs) if "(" in r and i != 5][:8]
        got, errs = gidx.plan_batch([qs[i] for i in sel], fuzzymatch=False, wildcardmatch=True)
        ref, errs_r = gidx.plan_batch([rs[i] for i in sel], fuzzymatch=False)
        assert errs == errs_r == [0] * len(sel)
        assert bytes(got)[:C.sizeof(N.GpuQuery) * len(sel)] == bytes(ref)[:C.sizeof(N.GpuQuery) * len(sel)]


# ---- 5. refresh ----------------------------------------------------------------------------

@ROUTES
def test_refresh(nxs, tmp_path, monkeypatch, route):
    ev = [("add", 10, ["apple", "maple", "zebra"]), ("add", 20, ["apple", "apply"]), ("add", 30, ["ample", "apple"]),
          ("add", 40, ["apply", "zebra"]), ("add", 50, ["ample"]), ("add", 60, ["apricot"]), ("rm", 60)]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 262144)
    open(d, "wb").write(dimg + b"\0" * 262144)
    gidx = nxs.open_files(t, d)
    set_route(monkeypatch, gidx, route)

    def truth_now():
        tr = px_truth_of_events(ev)
        return WildTruth(tr.terms, tr.dfs)

    def publish():
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        nxsfmt.publish_in_place(t, d, timg, dimg)
        return truth_now()
    try:
        pats = [b"*pl?", b"a*", b"*e", b"ap?*t", b"?ppl?"]
        assert gidx.wildcard_profile()["builds"] == 0               # never asked: nothing built
        before = check(gidx, truth_now(), pats, 5, "snapshot 0")
        assert before[0] == [(b"apple", 3, 3), (b"apply", 3, 2), (b"ample", 3, 2), (b"maple", 3, 1)]
        assert before[3] == [] and before[3].matches == 0           # its only doc is removed
        assert gidx.wildcard_profile()["builds"] == 1
        check(gidx, truth_now(), pats, 32, "again")
        assert gidx.wildcard_profile()["builds"] == 1               # repeated calls: no rebuild
        ev += [("rm", 20), ("rm", 40)]                              # every doc of "apply"
        after = check(gidx, publish(), pats, 5, "removal")
        assert b"apply" not in [t_ for t_, _, _ in after[0]] and after[0].matches == 3
        assert gidx.wildcard_profile()["builds"] == 2
        ev.append(("add", 70, ["applq", "zebra", "apricot"]))      # a new term, and a dead one comes back
        newer = check(gidx, publish(), pats, 5, "append")
        assert (b"applq", 3, 1) in newer[0] and newer[3] == [(b"apricot", 4, 1)]
        check(gidx, truth_now(), pats, 5, "again")
        assert gidx.wildcard_profile()["builds"] == 3
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 6. the call's surface, doc shards -----------------------------------------------------

@ROUTES
def test_api_surface_and_refusals(nxs, tmp_path, monkeypatch, route):
    term_dfs = [(b"hello", 2), (b"hallo", 3), (b"help", 1), (b"world", 1), (b"he", 1)]
    docs, _ = docs_of(term_dfs)
    t, d, term_ids = nxsfmt.write_index(str(tmp_path), "api", docs)
    truth = truth_of_docs(docs, (), term_ids)
    gidx = nxs.open_files(t, d, lowercase=True)
    try:
        with routed(monkeypatch, gidx, route):
            want = check(gidx, truth, [b"h?l*"], 5)[0]
            assert want == [(b"hallo", 3, 3), (b"hello", 3, 2), (b"help", 2, 1)] and want.matches == 3
            assert gidx.wildcard(["H?L*", "h?l**", "H?l***"]) == [want] * 3          # per piece, stars collapse
            L = N.lib()
            sg = L.nxs_index_wildcard(gidx._h, None, b"H?L*xyz", 4)                 # the length is the caller's
            assert sg and N._drain_sugg(sg) == want
            # a NUL within the length is a byte of the pattern (no term holds one)
            for pat, n in ((b"H?L*\0yz", 4), (b"HE\0LO*", 6), (b"\0H?L*", 5), (b"h?l*\0", 5),
                           (b"HELLO\0" + b"x" * 40 + b"*", 47)):
                sg = L.nxs_index_wildcard(gidx._h, None, pat, n)
                assert sg and N._drain_sugg(sg) == (want if n == 4 else []), (pat, n)
            doc = json.loads(gidx.wildcard(["H?L**"], json=True)[0])
            assert list(doc) == ["pattern", "terms", "matches"] and doc["pattern"] == "h?l*" and doc["matches"] == 3
            assert [(s["term"].encode(), s["df"]) for s in doc["terms"]] == [(t_, df) for t_, _, df in want]
            assert gidx.wildcard([]) == []
            for lim in (0, 33):
                with pytest.raises(N.NxsError) as e:
                    gidx.wildcard(["he*"], limit=lim)
                assert e.value.code == 3 and "wildcard_limit" in e.value.msg
                with pytest.raises(N.NxsError) as e:
                    gidx.search("h?", wildcardmatch=True, wildcard_terms=lim)
                assert e.value.code == 3 and "wildcard_terms" in e.value.msg
            got = gidx.wildcard(["h*o", "*", "??", "*?*", "", "a" * 256 + "?", "h?"])
            assert [isinstance(g, N.NxsError) and g.code for g in got] == [False, 3, 3, 3, 3, 3, False]
            assert got[0].matches == 2 and got[6] == [(b"he", 1, 1)]
            sg = L.nxs_index_wildcard(gidx._h, None, b"*", 1)
            assert not sg and nxs.error() == (3, "empty pattern")
            sg = L.nxs_index_wildcard(gidx._h, None, b"a" * 300 + b"*", 301)
            assert not sg and nxs.error() == (3, "wildcard pattern too long")
    finally:
        gidx.close()
    sh = nxs.open_shard(t, d, 0, 1)
    set_route(monkeypatch, sh, route)
    with pytest.raises(N.NxsError) as e:
        sh.wildcard(["he*"])
    assert e.value.code == 3 and e.value.msg == "wildcard is not available on a doc shard"
    with pytest.raises(N.NxsError) as e:
        nxs.docshard_search_batch([sh], ["hello", "h?llo AND world"], limit=5, wildcardmatch=True)
    assert e.value.code == 3 and e.value.msg == "wildcardmatch is not available on a doc shard"
    plain = nxs.docshard_search_batch([sh], ["hello", "world"], limit=5)
    assert nxs.docshard_search_batch([sh], ["hello", "world"], limit=5, wildcardmatch=True) == plain and plain[0]
    sh.close()
