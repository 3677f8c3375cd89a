"""GPU tier (`-m gpu`) for what the six blocking side passes share (nxs_gpu_side.hip): suggest, complete, wildcard,
explain, doc terms and related on ONE index of 2000 terms and 300 docs, each against the truth module its own test
file uses.  What is under test is the kit, not the kernels: the staging and the workspace grow and are used again,
profiling events are made by a later call than the one that made the stream, complete and wildcard share one term
order, everything is freed in the right order, and the two host rankers answer from one dictionary builder."""
import random

import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from complete_truth import Truth as PxTruth, random_words, truth_of_events
from explain_truth import check as check_explained
from related_truth import Truth as RtTruth, check_related
from similar_truth import Truth as DvTruth, check_vector
from suggest_truth import Truth as SgTruth, misspell
from wild_truth import WildTruth

pytestmark = pytest.mark.gpu

CALLS = ("suggest", "complete", "wildcard", "explain", "doc_terms", "related")
K = 5
N_TERMS, N_DOCS = 2000, 300


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


class World:
    """the files, the truths and, per call, distinct inputs (the first is the batch of one)"""


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """300 docs over a 2000-word a-f vocabulary (lengths 2-8): doc i holds words 7 i .. 7 i + 6 (every word is in
    some doc) and 8-16 Zipf-ish draws; three docs removed."""
    rng = random.Random(2300)
    vocab = [w.decode() for w in random_words(rng, N_TERMS, lo=2, hi=8)]
    weights = [1.0 / (1 + i) ** 0.7 for i in range(N_TERMS)]
    docs = []
    for i in range(N_DOCS):
        toks = [vocab[(7 * i + j) % N_TERMS] for j in range(7)] + rng.choices(vocab, weights, k=rng.randint(8, 16))
        docs.append((10 + 3 * i, toks))
    removed = [docs[i][0] for i in (3, 77, 250)]
    t, d, term_ids = nxsfmt.write_index(str(tmp_path_factory.mktemp("world")), "world", docs, removed=removed)
    assert len(term_ids) == N_TERMS
    w = World()
    w.t, w.d = t, d
    terms = [None] * N_TERMS
    for term, i in term_ids.items():
        terms[i - 1] = term
    w.dv = DvTruth(O.Index(t, d), docs, removed, term_ids)
    w.rt = RtTruth(w.dv.oidx, docs, removed, term_ids)
    dfs = [w.dv.df.get(term, 0) for term in terms]
    assert 0 < sum(1 for x in dfs if x == 0) < 40               # some terms live in removed docs only
    w.sg, w.px, w.wc = SgTruth(terms, dfs), PxTruth(terms, dfs), WildTruth(terms, dfs)
    live = [x for x in vocab if dfs[term_ids[x.encode()] - 1] > 0]
    words = rng.sample(live, 160)
    w.inputs = {
        "suggest": list(dict.fromkeys(misspell(rng, x.encode()) for x in words)),
        "complete": list(dict.fromkeys(x[:3].encode() for x in words)),
        "wildcard": list(dict.fromkeys((x[:2] + "*" + x[-1]).encode() for x in words)),
        "explain": ["%s OR %s" % (a, b) for a, b in zip(words, words[1:])],
        "doc_terms": [did for did, _ in docs if did not in removed],
        "related": ["%s OR %s" % (a, b) for a, b in zip(words[:32], words[32:])],
    }
    return w


def run(gidx, w, call, xs):
    """one batch of `call` over inputs xs, every answer against the truth -> something comparable"""
    if call == "suggest":
        got = gidx.suggest(xs, limit=K, maxdist=2)
        for x, g in zip(xs, got):
            want, m = w.sg.rank_terms(x, K, 2)
            assert list(g) == want and g.matches == m, (call, x)
    elif call in ("complete", "wildcard"):
        got = gidx.complete(xs, limit=K) if call == "complete" else gidx.wildcard(xs, limit=K)
        truth = w.px if call == "complete" else w.wc
        for x, g in zip(xs, got):
            want, m = truth.rank_terms(x, K)
            assert list(g) == want and g.matches == m, (call, x)
    elif call == "explain":
        plain = gidx.search_batch(xs, limit=10, fuzzymatch=False)
        got = gidx.search_batch(xs, limit=10, fuzzymatch=False, explain=True)
        for x, g, p in zip(xs, got, plain):
            assert check_explained(g, p, w.dv.ex, x, O.BM25, False, call) > 0, x
        return [(list(g), g.tokens, g.explain) for g in got]
    elif call == "doc_terms":
        got = gidx.doc_terms(xs, limit=K, mindf=1, algo="BM25")
        for x, g in zip(xs, got):
            check_vector(g, w.dv.rank(x, O.BM25, K, 1), (call, x))
    else:
        got = gidx.related(xs, limit=K, fuzzymatch=False, algo="BM25")
        for x, g in zip(xs, got):
            check_related(g, w.rt.related(x, O.BM25, K), (call, x))
        return [(list(g), g.matches, g.docs) for g in got]
    assert len(got) == len(xs)
    return [(list(g), g.matches) for g in got]


# ---- the passes' own size formulas: (staging, workspace) bytes of one pass over n inputs of `blen` bytes --------

def al(n, a):
    return (n + a - 1) // a * a


def carve(p, n):
    return al(p, 256) + n


def need_term_list(n, blen, wildcard):
    dn = al((n * K + n) * 8, 16)
    if wildcard:
        o_pb = n * 16 + (n + 1) * 4
        up = al(al(o_pb + blen, 16) + blen + 16, 16)
        return up + dn, up + dn + n * 8 + n * 64 * K * 8 + 1024
    up = al((n + 1) * 4 + blen + 16, 16)
    return up + dn, up + dn + n * 8 + 1024


def need_suggest(n, blen):
    up = al((2 * n + 1 + 64 + 2) * 4, 16)
    dn = al((2 * n * K + 2 * n + 4 + 64 * 16) * 4 + n * K, 16)
    qcap = max(16, min((32 << 20) // 64, (((N_TERMS + 255) // 256 + 63) // 64) * 256 * n))      # (n < 256: one slice)
    ccap = qcap * 64
    mcap = ccap if n == 1 else max(1024, ccap // 4)
    return (up + al(blen + 16, 16) + dn + 64,
            ccap * 8 + mcap * 24 + dn + n * (256 * 8 + 16) + 64 + up + blen + 16 + 16 * 256)


def need_explain(n, blen):
    """n two-token queries with one result each at least (a lower bound of what the call stages)"""
    pin = al(n * 24, 256) + al(2 * n * 24, 256) + al(n * 8, 256) + 2 * al(2 * n * 4, 256) + al(n, 256) + 256
    return pin, pin + 256


def need_doc_terms(n, blen):
    """(the bitmap terms' array is a constant of the index: the whole dictionary at most)"""
    per_doc = min(512, (N_TERMS + 63) // 64) * K * 8
    pin = 2 * al(n * 8, 256) + al(N_TERMS * 4 + 4, 256) + al(n * 4, 256) + 4 * al(n * K * 4, 256) + 2 * al(n * 4, 256)
    return pin, pin + n * per_doc + 512


def need_related(n, blen):
    g = min(32, n)
    p = 0
    for size in (g * 64, g * 2 * 32 * 8, g * 256, g * 8, g * 132, g * K * 4, g * K * 4, g * K * 4, g * 4, g * 4, g * 4):
        p = carve(p, size)
    row = (N_TERMS + 1) * 4
    ws = al(p, 256) + al(N_DOCS * 4, 256) + al(g * row, 256) + g * min(64, (N_TERMS + 255) // 256) * K * 8 + 512
    return p + 512, ws


NEED = {"suggest": need_suggest, "complete": lambda n, b: need_term_list(n, b, False),
        "wildcard": lambda n, b: need_term_list(n, b, True), "explain": need_explain, "doc_terms": need_doc_terms,
        "related": need_related}


def grown(call, xs):
    """the smallest batch xs[:n] whose pass needs more than 1.5 times the staging AND the workspace of xs[:1]'s"""
    size = lambda ys: sum(len(y) for y in ys) if isinstance(ys[0], (bytes, str)) else 0
    pin1, ws1 = NEED[call](1, size(xs[:1]))
    for n in range(2, len(xs) + 1):
        pin, ws = NEED[call](n, size(xs[:n]))
        if pin > 1.5 * pin1 and ws > 1.5 * ws1:
            return n
    raise AssertionError("%s: %d inputs do not outgrow one" % (call, len(xs)))


# ---- growth and reuse --------------------------------------------------------------------------------------

@pytest.mark.parametrize("call", CALLS)
def test_growth_and_reuse(nxs, world, call):
    """a batch of one on a fresh index (the buffers are made for it), a batch that outgrows both by more than half,
    the batch of one again in the grown buffers: all three are the truth"""
    xs = world.inputs[call]
    n = min(max(grown(call, xs), 8), len(xs))      # (8 at least: more than one row of every array)
    assert grown(call, xs) <= n
    gidx = nxs.open_files(world.t, world.d)
    try:
        first = run(gidx, world, call, xs[:1])
        many = run(gidx, world, call, xs[:n])
        assert run(gidx, world, call, xs[:1]) == first == many[:1]
    finally:
        gidx.close()


# ---- events made late --------------------------------------------------------------------------------------

PASSES = {"suggest": ("suggest_profile", "passes", "ms"), "complete": ("complete_profile", "passes", "ms"),
          "wildcard": ("wildcard_profile", "passes", "ms"), "explain": ("explain_profile", "passes", "ms"),
          "doc_terms": ("doc_terms_profile", "passes", "scan_ms"), "related": ("related_profile", "passes", "scan_ms")}


@pytest.mark.parametrize("call", CALLS)
def test_events_made_late(nxs, world, call):
    """the first call with profiling off makes the stream and no events; profiling switched on, the second call
    makes them, answers the same and is timed: its one pass is counted"""
    xs = world.inputs[call][:3]
    prof_of, passes, ms = PASSES[call]
    gidx = nxs.open_files(world.t, world.d)
    try:
        gidx.set_profiling(False)
        first = run(gidx, world, call, xs)
        before = getattr(gidx, prof_of)()
        assert before[ms] == 0.0, before
        gidx.set_profiling(True)
        assert run(gidx, world, call, xs) == first
        after = getattr(gidx, prof_of)()
        # (the explain test runs the batch twice, with and without explanations: one pass all the same)
        assert after[passes] - before[passes] == 1, (before, after)
        assert after[ms] > 0.0, after
    finally:
        gidx.set_profiling(False)
        gidx.close()


# ---- the shared order ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", ["complete", "wildcard"])
def test_shared_order(nxs, tmp_path, first):
    """complete, wildcard, complete on one index build the order once; after a refresh it is built once more,
    whichever of the two asks first"""
    ev = [("add", 10, ["apple", "maple", "zebra"]), ("add", 20, ["apple", "apply"]), ("add", 30, ["ample", "apple"])]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 262144)
    open(d, "wb").write(dimg + b"\0" * 262144)
    gidx = nxs.open_files(t, d)

    def ask(call, truth):
        if call == "complete":
            xs, got, tr = [b"ap", b"z"], gidx.complete([b"ap", b"z"], limit=K), truth
        else:
            xs, got, tr = [b"a*e", b"?ebra"], gidx.wildcard([b"a*e", b"?ebra"], limit=K), WildTruth(truth.terms, truth.dfs)
        for x, g in zip(xs, got):
            assert (list(g), g.matches) == tr.rank_terms(x, K), (call, x)
        return gidx.complete_profile()["builds"], gidx.wildcard_profile()["builds"]
    try:
        assert gidx.complete_profile()["builds"] == 0
        truth = truth_of_events(ev)
        for call in ("complete", "wildcard", "complete"):
            assert ask(call, truth) == (1, 1)
        ev += [("rm", 20), ("add", 40, ["applq", "zebra"])]
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        nxsfmt.publish_in_place(t, d, timg, dimg)
        truth = truth_of_events(ev)
        other = "wildcard" if first == "complete" else "complete"
        for call in (first, other, first):
            assert ask(call, truth) == (2, 2)
    finally:
        gidx.close()


# ---- teardown ------------------------------------------------------------------------------------------------

def test_teardown_after_all_six(nxs, world):
    """an index on which all six passes have run (with their events) closes -- the wildcard state before the
    prefix state whose stream it borrows -- and the next index on the same files answers"""
    gidx = nxs.open_files(world.t, world.d)
    gidx.set_profiling(True)
    want = {call: run(gidx, world, call, world.inputs[call][:2]) for call in CALLS}
    gidx.set_profiling(False)
    gidx.close()
    again = nxs.open_files(world.t, world.d)
    try:
        for call in ("wildcard", "complete") + CALLS:
            assert run(again, world, call, world.inputs[call][:2]) == want[call]
    finally:
        again.close()


# ---- host routes -----------------------------------------------------------------------------------------------

def test_host_routes_share_one_dictionary(nxs, world, monkeypatch):
    """NXS_GPU_SUGGEST=host and NXS_GPU_COMPLETE=host: both rankers answer from the one dictionary builder, and as
    the device passes do"""
    gidx = nxs.open_files(world.t, world.d)
    try:
        dev = {call: run(gidx, world, call, world.inputs[call][:40]) for call in ("suggest", "complete")}
        monkeypatch.setenv("NXS_GPU_SUGGEST", "host")
        monkeypatch.setenv("NXS_GPU_COMPLETE", "host")
        gidx.reconfigure()
        for call in ("suggest", "complete"):
            assert run(gidx, world, call, world.inputs[call][:40]) == dev[call]
        live = sum(1 for x in world.px.dfs if x > 0)
        assert gidx.suggest_profile()["host_tokens"] == 40 and gidx.complete_profile()["host_prefixes"] == 40
        assert gidx.complete_profile()["entries"] == live       # the dictionary: every term with df > 0
    finally:
        monkeypatch.delenv("NXS_GPU_SUGGEST")
        monkeypatch.delenv("NXS_GPU_COMPLETE")
        gidx.reconfigure()
        gidx.close()
