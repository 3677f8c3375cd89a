"""GPU tier (`-m gpu`): the term-side device state, read back array by array (Index.term_image) and compared
with the host model of tests/term_truth.py -- the BK image, the side arrays and candidates of the match-first fuzzy
search, suggest's candidates and the byte order that completion and wildcard matching read -- on a fresh load and
after each of four refreshes of one index: removals only (a flag and two df move), appends without a new term
(only df moves: the BK image must stay, the order's keys must not), appends with new terms (one of them next to
the root: BFS renumbers nearly every node), and a doc id below the highest loaded one (the full rebuild).

Answers of suggest, complete, wildcard and the fuzzy search see this state only through the tokens a test asks: a
signature bit, a stale df in a key, two swapped entries of the order, a parent off by one leave them green.

The lazily built parts are read after the call that builds them, and the scalars are read before it too: right
after a refresh suggest's candidates and the order must be behind their generation, after the call they must be
level with it and the order must have been built exactly once.  Two walks: in the first the calls after a refresh
are a fuzzy search, a suggest and a complete; in the second a wildcard comes first (it brings the BK image up to
date itself and builds the order), then the suggest, then the fuzzy search.

tests/test_term_image_host.py asserts without a GPU that every designed edge is in the corpus and that the
checker names a wrong value in every array.  No mutated library is run here."""
import ctypes as C
import os
import random
import struct

import numpy as np
import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
import term_truth as TT

pytestmark = pytest.mark.gpu

FUZZY_Q = "ordexabcd"           # one edit from orderabcd, which no snapshot loses
SUGG_TOK = b"ordexab"
PREFIX, PATTERN = "sw", "sw*"
ARRAYS = [k for k in N.TIMG_PARTS]
SIZES = ("n_bk", "bk_depth", "bk_bytes_len", "n_fz", "sg_n_c", "px_n_e")


def model_of_files(t, d, ev=None):
    """the model of the snapshot the two files hold now: bytes and totals from nxsterms, df from the oracle"""
    terms, totals = TT.read_terms(t)
    oidx = O.Index(t, d)
    try:
        assert oidx.term_count == len(terms)
        assert all(oidx.term(i + 1) == w for i, w in enumerate(terms))
        dfs = [int(oidx.df(i + 1)) for i in range(len(terms))]
        hits = oidx.search(FUZZY_Q, limit=5)
    finally:
        oidx.close()
    if ev is not None:
        df = TT.live_df(ev)
        assert dfs == [df.get(w, 0) for w in terms]
    return TT.TermModel(terms, totals, dfs), hits


def stale(sc, what):
    return not (sc[what + "_built"] and sc[what + "_built_gen"] == sc[what + "_gen"])


def completions(m, prefix):
    """what complete / wildcard("<prefix>*") answer at the default limit: (term, extra bytes, df), df descending"""
    p = prefix.encode()
    rows = sorted((-m.dfs[i], i + 1) for i, w in enumerate(m.terms) if w.startswith(p) and m.dfs[i] > 0)
    return [(m.terms[i - 1], len(m.terms[i - 1]) - len(p), -ndf) for ndf, i in rows[:5]], len(rows)


def same_hits(got, want, ctx):
    assert [(d, struct.pack("<f", s)) for d, s in got] == [(d, struct.pack("<f", s)) for d, s in want], ctx


def three_calls(gidx, order):
    """-> {call: (answer, the image read right after it)}"""
    out = {}
    for call in order:
        if call == "fuzzy":
            ans = gidx.search(FUZZY_Q, limit=5, fuzzymatch=True)
        elif call == "suggest":
            g = gidx.suggest([SUGG_TOK])[0]
            ans = (list(g), g.matches)
        else:
            g = (gidx.complete([PREFIX]) if call == "complete" else gidx.wildcard([PATTERN]))[0]
            ans = (list(g), g.matches)
        out[call] = (ans, gidx.term_image())
    return out


class Walk:
    """One index through the five snapshots, in order; every step keeps its images and its model."""

    def __init__(self, base, order):
        self.order = order
        self.ev, self.cut, self.zero, self.info = TT.corpus()
        # before any comparison: every designed edge is in the corpus, or nothing below runs
        TT.preconditions(TT.event_models(self.ev, self.cut, self.zero), self.info)
        self.nxs = N.Nxs(str(base))
        self.t, self.d = str(base / "nxsterms"), str(base / "nxsdtmap")
        timg, dimg = TT.images(self.ev[:self.cut[0]], self.zero[0])
        # room for the appends: the files are sized once, like a preallocated index
        open(self.t, "wb").write(timg + b"\0" * (1 << 16))
        open(self.d, "wb").write(dimg + b"\0" * (1 << 16))
        self.gidx = self.nxs.open_files(self.t, self.d)
        self.snap, self.error = [], None

    def upto(self, k):
        if self.error is not None:
            pytest.fail("an earlier snapshot failed: %r" % (self.error,))
        while len(self.snap) <= k:
            try:
                self.snap.append(self.step(len(self.snap)))
            except BaseException as e:
                self.error = e
                raise
        return self.snap[k]

    def step(self, k):
        ev = self.ev[:self.cut[k]]
        if k:
            timg, dimg = TT.images(ev, self.zero[k])
            nxsfmt.publish_in_place(self.t, self.d, timg, dimg)
        # a search without a fuzzy token picks the refresh up and touches nothing of the term side
        assert len(self.gidx.search("all", limit=5)) == 5
        s = {"after_refresh": self.gidx.term_image()["scalars"]}
        # (the oracle maps the files, which the next step rewrites in place: everything is asked of it now)
        s["model"], s["want_hits"] = model_of_files(self.t, self.d, ev)
        s["calls"] = three_calls(self.gidx, self.order)
        fresh = self.nxs.open_files(self.t, self.d)
        try:
            s["fresh"] = three_calls(fresh, self.order)
        finally:
            fresh.close()
        # the host rankers, on the refreshed index: their dictionary is a copy of the same snapshot
        old = {e: os.environ.get(e) for e in ("NXS_GPU_SUGGEST", "NXS_GPU_COMPLETE")}
        try:
            os.environ.update({"NXS_GPU_SUGGEST": "host", "NXS_GPU_COMPLETE": "host"})
            self.gidx.reconfigure()
            g, c = self.gidx.suggest([SUGG_TOK])[0], self.gidx.complete([PREFIX])[0]
            s["host"] = {"suggest": (list(g), g.matches), "complete": (list(c), c.matches)}
        finally:
            for e, v in old.items():
                os.environ.pop(e, None) if v is None else os.environ.__setitem__(e, v)
            self.gidx.reconfigure()
        s["end"] = self.gidx.term_image()
        stats = (C.c_uint64 * 2)()
        L = N.lib()
        L.nxs_index_refresh_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.nxs_index_refresh_stats(self.gidx._h, stats)
        s["stats"] = (int(stats[0]), int(stats[1]))
        return s

    def close(self):
        self.gidx.close()
        self.nxs.close()


ORDERS = {"fuzzy-suggest-complete": ("fuzzy", "suggest", "complete"),
          "wildcard-suggest-fuzzy": ("wildcard", "suggest", "fuzzy")}


@pytest.fixture(scope="module", params=list(ORDERS))
def walk(request, tmp_path_factory):
    w = Walk(tmp_path_factory.mktemp("terms"), ORDERS[request.param])
    yield w
    w.close()


def test_the_corpus_holds_every_designed_edge(walk):
    """From the models the walk compares with (bytes and totals from the files, df from the oracle): a test that
    cannot find its edge fails here."""
    TT.preconditions([walk.upto(k)["model"] for k in range(5)], walk.info)


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_term_image_of_the_refreshed_index_equals_the_model(walk, k):
    """Snapshot 0 is the fresh load of the index that then takes the refreshes (1: removals only, 2: appends without a
    new term, 3: appends with new terms, 4: the full rebuild): the generations right after the refresh and after
    every call, every part built so far against the model, the answers, and the host rankers' answers."""
    s = walk.upto(k)
    m, calls, order = s["model"], s["calls"], walk.order
    assert s["stats"] == ((k, 0) if k < 4 else (3, 1)), s["stats"]
    r = s["after_refresh"]
    prev = walk.snap[k - 1] if k else None
    # ---- right after the refresh: both lazily built parts are behind, nothing of the BK image has moved yet
    assert stale(r, "sg") and stale(r, "px"), (k, "built before any side call", r)
    if k in (1, 2, 3):
        p = prev["end"]["scalars"]
        assert (r["sg_gen"], r["px_gen"]) == (p["sg_gen"] + 1, p["px_gen"] + 1), (k, "generations after the refresh", p, r)
        assert [r[x] for x in SIZES[:4]] == [p[x] for x in SIZES[:4]], (k, "the BK image moved before a call asked", p, r)
        # the image goes up again only when a term was added or a "total > 0" flag moved
        up = m.terms != prev["model"].terms or not np.array_equal(m.bk["flags"], prev["model"].bk["flags"])
        assert up == (k != 2)
    else:
        up = False                  # a new device index: the image came with it
        assert r["px_builds"] == 0 and not r["sg_built"] and not r["px_built"], (k, r)
    # ---- call by call
    gen = r["sg_gen"] + (1 if up else 0)
    built = set()
    for call in order:
        ans, img = calls[call]
        sc = img["scalars"]
        ctx = (k, "after " + call)
        assert (sc["sg_gen"], sc["px_gen"]) == (gen, r["px_gen"] + (1 if up else 0)), (ctx, "generations", r, sc)
        built.add({"fuzzy": "bk", "suggest": "sg", "complete": "px", "wildcard": "px"}[call])
        assert stale(sc, "sg") == ("sg" not in built) and stale(sc, "px") == ("px" not in built), (ctx, "lazy rebuild", sc)
        assert sc["px_builds"] == r["px_builds"] + (1 if "px" in built else 0), (ctx, "order builds", r, sc)
        # (every call brings the BK image up to date before it looks at it)
        TT.check_term_image(img, m, ctx, parts=("bk", "fz") + tuple(x for x in ("sg", "px") if x in built))
    # ---- the answers
    same_hits(calls["fuzzy"][0], s["want_hits"], (k, "fuzzy search"))
    assert calls["fuzzy"][0], (k, "the fuzzy query must have hits")
    assert calls["complete" if "complete" in order else "wildcard"][0] == completions(m, PREFIX), k
    names = [w for w, _, _ in completions(m, PREFIX)[0]]
    assert names == ([walk.info["swa"], walk.info["swb"]] if k < 2 else [walk.info["swb"], walk.info["swa"]])
    # ---- the host rankers answer the same from their copy of the snapshot; that copy is one more build
    assert s["host"]["suggest"] == calls["suggest"][0], (k, "suggest: host route against device route")
    assert s["host"]["complete"] == completions(m, PREFIX), (k, "complete: host route")
    assert s["end"]["scalars"]["px_builds"] == r["px_builds"] + 2, (k, s["end"]["scalars"])
    for name in ARRAYS:
        assert np.array_equal(s["end"][name], calls[order[-1]][1][name]), (k, name, "moved under the host route")


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_term_image_of_a_fresh_load_equals_the_refreshed_one(walk, k):
    """A second index opened fresh on the same files, after the same three calls: the model, and every array and
    size equal to the refreshed index's."""
    s = walk.upto(k)
    last = walk.order[-1]
    fimg, img = s["fresh"][last][1], s["calls"][last][1]
    TT.check_term_image(fimg, s["model"], (k, "fresh"))
    assert fimg["scalars"]["px_builds"] == 1
    for name in ARRAYS:
        assert np.array_equal(fimg[name], img[name]), (k, name, "fresh against refreshed")
    assert [fimg["scalars"][x] for x in SIZES] == [img["scalars"][x] for x in SIZES], k
    for call in walk.order:
        assert s["fresh"][call][0] == s["calls"][call][0] or call == "fuzzy", (k, call)
    same_hits(s["fresh"]["fuzzy"][0], s["want_hits"], (k, "fresh fuzzy search"))


def tiny(name):
    """three dictionaries for the grid edges the walk does not reach: no live term, a single term, and 256 terms,
    all live (one full block of every kernel that builds this state)"""
    if name == "none":
        return [("add", 5, [b"abc", b"abd", b"xyz"]), ("add", 6, [b"abcd", b"q", b"orderabcd"]), ("rm", 5), ("rm", 6)]
    if name == "one":
        return [("add", 5, [b"orderabcd"]), ("add", 6, [b"orderabcd"])]
    rng = random.Random(256)
    words = [b"orderabcd", b"swa", b"swb"] + TT._words(rng, 253, b"abcdef", 2, 9, {b"orderabcd", b"swa", b"swb"})
    return [("add", 10 + j, words[8 * j:8 * j + 8] + [b"swa"]) for j in range(32)]


@pytest.mark.parametrize("name,live", [("none", 0), ("one", 1), ("256", 256)])
def test_tiny_dictionaries_at_a_fresh_load(tmp_path, name, live):
    ev = tiny(name)
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "t"), str(tmp_path / "d")
    open(t, "wb").write(timg)
    open(d, "wb").write(dimg)
    m, want_hits = model_of_files(t, d, ev)
    assert len(m.px) == len(m.sg) == live and (name != "256" or m.n == len(m.fz) == 256) and (name != "one" or m.n == 1)
    with N.Nxs(str(tmp_path)) as nxs:
        gidx = nxs.open_files(t, d)
        try:
            calls = three_calls(gidx, ORDERS["fuzzy-suggest-complete"])
        finally:
            gidx.close()
    TT.check_term_image(calls["complete"][1], m, (name, "fresh"))
    same_hits(calls["fuzzy"][0], want_hits, name)
    assert calls["complete"][0] == completions(m, PREFIX), name
    if not live:
        for part in ("sg_node", "sg_sig", "sg_len", "px_node", "px_key"):
            assert calls["complete"][1][part].size == 0, (name, part)


def test_term_image_hook_refuses_batches_in_flight_and_changes_nothing(tmp_path):
    """The hook itself: parts that no call has built yet are empty and the scalars say so; an error while a batch is
    in flight; reading twice gives the same bytes and builds nothing."""
    ev = tiny("256")
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "t"), str(tmp_path / "d")
    open(t, "wb").write(timg)
    open(d, "wb").write(dimg)
    m, _ = model_of_files(t, d, ev)
    with N.Nxs(str(tmp_path)) as nxs:
        gidx = nxs.open_files(t, d)
        a = gidx.term_image()
        assert not a["scalars"]["sg_built"] and not a["scalars"]["px_built"] and a["scalars"]["px_builds"] == 0
        for part in ("sg_node", "sg_sig", "sg_len", "px_node", "px_key"):
            assert a[part].size == 0, part
        TT.check_term_image(a, m, "before any call", parts=("bk", "fz"))      # the BK image comes with the load
        gidx.search_batch_begin(["swa", "orderabcd OR swb"], limit=10)
        with pytest.raises(N.NxsError, match="in flight"):
            gidx.term_image()
        assert len(gidx.search_batch_end()) == 2
        before = gidx.complete([PREFIX])[0]
        b, c = gidx.term_image(), gidx.term_image()
        assert b["scalars"] == c["scalars"] and b["scalars"]["px_builds"] == 1 and stale(b["scalars"], "sg")
        for name in ARRAYS:
            assert np.array_equal(b[name], c[name]), name
        assert list(gidx.complete([PREFIX])[0]) == list(before)
        assert gidx.term_image()["scalars"] == b["scalars"]
        gidx.close()
