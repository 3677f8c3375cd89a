"""GPU tier (`-m gpu`) for related terms: Index.related (nxs_index_related_batch, nxsgpu_related: k_rt_mask /
k_rt_scan / k_rt_select / k_rt_merge).

Truth is related_truth.py: the doc set from the CPU oracle with the limit lifted, the resolved token list of
explain_truth, c and df counted in Python from the docs the test wrote, s = numpy.float32(c / df).  Everything is
compared in full: terms, order, c, df, score bits, matches, docs.  Every test takes both routes -- the device
pass and NXS_GPU_RELATED=host -- and the profile's counters prove which one ran."""
import contextlib
import json
import random
import re

import numpy as np
import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from related_truth import Truth, check_related

pytestmark = pytest.mark.gpu

ROUTES = pytest.mark.parametrize("route", [None, "host"], ids=["device", "host"])
ALGOS = {"BM25": O.BM25, "TF-IDF": O.TF_IDF}
INVALID, LIMIT = 3, 6
ORDERS = ("count", "share")


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def set_route(monkeypatch, gidx, route, run=None, parts=None, ws=None):
    """NXS_GPU_RELATED: None = the device pass, "host" = the host loop; NXS_GPU_RELATED_RUN / _PARTS / _WS"""
    for key, v in (("NXS_GPU_RELATED", route), ("NXS_GPU_RELATED_RUN", run), ("NXS_GPU_RELATED_PARTS", parts),
                   ("NXS_GPU_RELATED_WS", ws)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(v))
    gidx.reconfigure()


@contextlib.contextmanager
def routed(monkeypatch, gidx, route, run=None, parts=None, ws=None):
    """the body's queries take `route`, and only that route: the profile's counters say so"""
    set_route(monkeypatch, gidx, route, run, parts, ws)
    gidx.related_profile(reset=True)
    try:
        yield
        prof = gidx.related_profile()
        took, other = ("device_queries", "host_queries") if route is None else ("host_queries", "device_queries")
        assert prof[took] > 0 and prof[other] == 0, (route, prof)
        assert (prof["passes"] > 0) == (route is None), (route, prof)
    finally:
        set_route(monkeypatch, gidx, None)


def make(path, name, docs, removed=()):
    t, d, term_ids = nxsfmt.write_index(str(path), name, docs, removed=removed)
    return t, d, Truth(O.Index(t, d), docs, removed, term_ids)


def check(gidx, truth, qs, algo="BM25", k=5, order=None, mindf=None, mincount=None, include_self=None,
          fuzzymatch=False, ctx=None):
    """one Index.related batch against the truth; a query the oracle rejects must be rejected with its code"""
    got = gidx.related(qs, limit=k, order=order, mindf=mindf, mincount=mincount, include_self=include_self,
                       fuzzymatch=fuzzymatch, algo=algo)
    assert len(got) == len(qs)
    for q, g in zip(qs, got):
        c = (ctx, q[:70], algo, k, order, mindf, mincount, include_self, fuzzymatch)
        try:
            want = truth.related(q, ALGOS[algo], k, order or "count", mindf or 1, mincount or 1, bool(include_self),
                                 fuzzymatch)
        except O.SearchError as e:
            assert isinstance(g, N.NxsError) and g.code == e.code, (c, g)
            continue
        check_related(g, want, c)
    return got


def random_query(rng, vocab, nmax):
    q = rng.choice(vocab)
    for _ in range(rng.randint(1, nmax) - 1):
        q += rng.choice([" AND ", " OR ", " AND NOT ", " "]) + rng.choice(vocab)
    return q


# ---- 1. mask tile seams -------------------------------------------------------------------------------

def tile_widths():
    import ctypes as C
    w = (C.c_uint32 * 2)()
    L = N.lib()
    L.nxs_test_count_tile_widths.argtypes = [C.POINTER(C.c_uint32)]
    L.nxs_test_count_tile_widths(w)
    return int(w[0]), int(w[1])


@pytest.fixture(scope="module")
def seam_corpora(tmp_path_factory):
    """n docs of two or three tokens: `all` in every doc, `last` only in the last doc of the first tile, `first`
    only in the first doc of the second, `tail` only in the last doc; built once per n, shared by the routes"""
    made = {}

    def get(W, n):
        if n not in made:
            rng = random.Random(n)
            vocab = ["v%d" % i for i in range(12)]
            docs, did = [], 0
            for i in range(n):
                did += rng.randint(1, 1000)
                toks = [rng.choice(vocab) for _ in range(rng.randint(1, 2))] + ["all"]
                if i == W - 1:
                    toks.append("last")
                if i == W:
                    toks.append("first")
                if i == n - 1:
                    toks.append("tail")
                docs.append((did, toks))
            made[n] = make(tmp_path_factory.mktemp("seam%d" % n), "seam", docs) + (vocab,)
        return made[n]
    return get


@ROUTES
@pytest.mark.parametrize("size", ["W-1", "W", "W+1", "2W+1"])
@pytest.mark.parametrize("which", [0, 1], ids=["u8", "u32"])
def test_mask_tile_seams(nxs, seam_corpora, monkeypatch, route, which, size):
    """Corpora that end just before, on and just behind a boundary of the mask tile (both widths); queries of 1, 2,
    8 and 9 tokens (the last take the postfix program), AND / OR / AND NOT, every doc, no doc; .docs is the total"""
    W = tile_widths()[which]
    assert W == (16384, 4096)[which]
    n = {"W-1": W - 1, "W": W, "W+1": W + 1, "2W+1": 2 * W + 1}[size]
    t, d, truth, vocab = seam_corpora(W, n)
    gidx = nxs.open_files(t, d)
    qs = ["all", "last", "first", "tail", "v3", "v1 AND v2", "v1 OR last", "all AND NOT last", "all AND NOT first",
          "first OR tail", "last AND first", "v0 AND NOT all", "nosuchterm", "tail AND NOT v1",
          " OR ".join(vocab[:8]), "(" + " OR ".join(vocab[:7]) + ") AND NOT last",
          " OR ".join(vocab[:9]), "(" + " OR ".join(vocab[:9]) + ") AND NOT first", " OR ".join(vocab) + " OR last OR first",
          "(" + " OR ".join(vocab[:10]) + ") AND (last OR first OR tail)", " OR ".join(vocab) + " OR all"]
    try:
        with routed(monkeypatch, gidx, route):
            got = check(gidx, truth, qs, k=32, ctx=(size, W))
            check(gidx, truth, qs[5:9] + qs[15:18], k=5, order="share", include_self=True, ctx=(size, W, "share"))
            totals = gidx.search_batch(qs, limit=1, fuzzymatch=False, total=True)
            assert [g.docs for g in got] == [x.total for x in totals]
            assert got[0].docs == n and got[-1].docs == n and got[12].docs == 0 and list(got[12]) == []
            assert got[1].docs == (1 if n >= W else 0) and got[2].docs == (1 if n > W else 0) and got[3].docs == 1
            assert got[10].docs == 0 and got[10].matches == 0
    finally:
        gidx.close()


# ---- 2. scan seams ------------------------------------------------------------------------------------

RUN = 64            # NXS_GPU_RELATED_RUN at its smallest legal value: one wavefront's worth


@pytest.fixture(scope="module")
def lists(tmp_path_factory):
    """Term ids follow the first doc's token order and the flat posting array is in term-id order, so at a run of
    64 postings: A (64 postings) fills run 0 and ends on its boundary, B (1) begins exactly at run 1's first posting,
    C (63) ends on run 1's last, D (65) crosses into run 3, E (3 x 64 + 1 = 193) begins at posting 193 and spans four
    workgroups.  qa / qb / pad are the query side.  Doc 5 holds D three times."""
    lens = (("A", 64), ("B", 1), ("C", 63), ("D", 65), ("E", 3 * RUN + 1))
    docs = []
    for i in range(1, 201):
        toks = [name for name, ln in lens if i <= ln]
        if i == 5:
            toks += ["D", "D"]
        if i == 1 or i % 2:
            toks.append("qa")
        if i == 1 or i % 3 == 0:
            toks.append("qb")
        toks.append("pad")
        docs.append((i, toks))
    t, d, truth = make(tmp_path_factory.mktemp("lists"), "lists", docs)
    assert [truth.term_ids[x.encode()] for x, _ in lens] == [1, 2, 3, 4, 5]
    assert [truth.df[x.encode()] for x, _ in lens] == [ln for _, ln in lens]
    assert truth.ex.tf[b"D"][5] == 3
    return t, d, truth


@ROUTES
@pytest.mark.parametrize("run", [RUN, None], ids=["run64", "default-run"])
def test_scan_seams(nxs, lists, monkeypatch, route, run):
    t, d, truth = lists
    gidx = nxs.open_files(t, d)
    qs = ["qa", "qb", "qa OR qb", "qa AND NOT qb", "pad", "pad AND NOT qa", "B", "E AND NOT D", "C OR qb"]
    try:
        with routed(monkeypatch, gidx, route, run=run):
            for order in ORDERS:
                got = check(gidx, truth, qs, k=32, order=order, ctx=("lists", run))
                check(gidx, truth, qs, k=32, order=order, include_self=True, ctx=("lists self", run))
            rows = {x[0]: x for x in gidx.related(["pad"], limit=32, fuzzymatch=False)[0]}
            assert [rows[x][1:3] for x in (b"A", b"B", b"C", b"D", b"E")] == [(64, 64), (1, 1), (63, 63), (65, 65), (193, 193)]
            assert got[4].docs == 200
            # a doc that holds a term three times counts once: doc 5 is odd, D is in docs 1 .. 65
            rows = {x[0]: x for x in gidx.related(["qa"], limit=32, fuzzymatch=False)[0]}
            assert rows[b"D"][1:3] == (33, 65)
    finally:
        gidx.close()


# ---- 3. groups and passes, 4. selection ---------------------------------------------------------------

@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """300 docs of three words over a 700-word vocabulary (three 256-term tiles) plus 12 frequent words v0 .. v11"""
    rng = random.Random(700)
    vocab = ["v%d" % i for i in range(12)]
    rare = ["w%d" % i for i in range(700)]
    docs = [(10 + 3 * i, [rng.choice(vocab), rng.choice(vocab)] + rng.sample(rare, 3)) for i in range(300)]
    # designed ties under "share": 2/4, 3/6 and 1/2 of the docs that hold `probe`
    for j, (c, df) in enumerate(((2, 4), (3, 6), (1, 2), (3, 3), (3, 5))):
        for i in range(df):
            docs.append((5000 + 10 * j + i, ["tie%d" % j] + (["probe"] if i < c else ["other"])))
    return make(tmp_path_factory.mktemp("wide"), "wide", docs) + (vocab, rare)


@ROUTES
@pytest.mark.parametrize("ws", [None, 1, 3], ids=["default", "G1", "G3"])
def test_groups_and_passes(nxs, wide, monkeypatch, route, ws):
    """Batches of 1, 31, 32, 33 and 70 queries; NXS_GPU_RELATED_WS small enough for groups of 1 and 3 plans; the same
    string twice, two strings with one plan, a parse error and a query of 33 terms in the middle"""
    t, d, truth, vocab, rare = wide
    rng = random.Random(70)
    gidx = nxs.open_files(t, d)
    row = (len(truth.term_ids) + 1) * 4
    with pytest.raises(O.SearchError) as oe:
        truth.doc_set("broken AND", O.BM25)
    bad_code = oe.value.code
    live = [w for w in rare if w.encode() in truth.df]
    assert len(live) >= 33
    try:
        with routed(monkeypatch, gidx, route, ws=None if ws is None else ws * row):
            for n in (1, 31, 32, 33, 70):
                qs = ["v1 OR v2"] if n == 1 else []
                while len(qs) < n:
                    q = random_query(rng, vocab + rare[:20], 4)
                    if q not in qs:
                        qs.append(q)
                if n > 4:
                    qs[n // 2] = qs[0]                                  # the same string twice
                    qs[n // 2 + 1] = "  " + qs[1]                       # another string, the same plan
                    qs[n // 3] = "broken AND"
                    qs[n // 3 + 1] = " OR ".join(live[:33])             # 33 live tokens: a search's wide plan
                gidx.related_profile(reset=True)
                got = gidx.related(qs, limit=8, fuzzymatch=False)
                prof = gidx.related_profile()
                for i, (q, g) in enumerate(zip(qs, got)):
                    if q == "broken AND":
                        assert isinstance(g, N.NxsError) and g.code == bad_code, (n, i, g)
                    elif q.count(" OR ") == 32:
                        assert isinstance(g, N.NxsError) and g.code == LIMIT, (n, i, g)
                    else:
                        check_related(g, truth.related(q.strip(), O.BM25, 8), ("batch", n, i, q))
                if n > 4:
                    assert got[n // 2] == got[0] and got[n // 2 + 1] == got[1] and got[n // 2 + 1].docs == got[1].docs
                served = prof["device_queries"] + prof["host_queries"]
                assert served <= n - (4 if n > 4 else 0), (n, prof)      # identical plans are answered once
                assert served > 0 or n > 1, (n, prof)
                if route is None and ws:
                    assert prof["passes"] == (served + ws - 1) // ws, (n, ws, prof)
                elif route is None:
                    assert prof["passes"] == (served + 31) // 32, (n, prof)
            assert gidx.related([]) == []
            with pytest.raises(N.NxsError) as e:
                N._drain_related(N.lib().nxs_index_related(gidx._h, None, b"broken AND", 10) or gidx.nxs._raise())
            assert e.value.code == bad_code
            gidx.related(["v1"], fuzzymatch=False)
    finally:
        gidx.close()


@ROUTES
@pytest.mark.parametrize("k", [1, 5, 32])
def test_selection(nxs, wide, monkeypatch, route, k):
    """k = 1, 5, 32 with NXS_GPU_RELATED_PARTS = 3 over three tiles of terms; matches below k; ties in c and in the
    share decided by the term id; mincount and mindf at the value that admits a term and one above it"""
    t, d, truth, vocab, rare = wide
    gidx = nxs.open_files(t, d)
    qs = ["probe", "v1 OR v2 OR v3", "v1 AND v2", "other AND NOT probe", "probe OR other", "tie3", rare[5]]
    try:
        with routed(monkeypatch, gidx, route, parts=3):
            for order in ORDERS:
                check(gidx, truth, qs, k=k, order=order, ctx="sel")
                for mindf, mincount in ((2, 1), (3, 1), (4, 2), (1, 3), (1, 4), (6, 3), (7, 3)):
                    check(gidx, truth, qs, k=k, order=order, mindf=mindf, mincount=mincount, ctx="floors")
            full = gidx.related(["probe"], limit=32, order="share", fuzzymatch=False)[0]
            shares = [(x[0], x[1], x[2]) for x in full if x[0].startswith(b"tie")]
            # 3/3 first, then 3/5, then the three shares of exactly one half by term id: 2/4, 3/6, 1/2
            assert shares == [(b"tie3", 3, 3), (b"tie4", 3, 5), (b"tie0", 2, 4), (b"tie1", 3, 6), (b"tie2", 1, 2)]
            assert len({x[3] for x in full if x[0] in (b"tie0", b"tie1", b"tie2")}) == 1
            full = gidx.related(["probe"], limit=32, fuzzymatch=False)[0]
            assert [x[0] for x in full] == [b"tie1", b"tie3", b"tie4", b"tie0", b"tie2"] and full.matches == 5 and full.docs == 12
            # the floors: tie0 (c 2, df 4) is admitted at mincount 2 / mindf 4 and not one above
            for kw, n in (({"mincount": 2}, 4), ({"mincount": 3}, 3), ({"mindf": 4}, 3), ({"mindf": 5}, 2)):
                g = gidx.related(["probe"], limit=32, fuzzymatch=False, **kw)[0]
                assert g.matches == n == len(g) and (b"tie0" in [x[0] for x in g]) == (kw in ({"mincount": 2}, {"mindf": 4}))
            for key, kw, bad in (("related_limit", "limit", (0, 33)), ("related_mindf", "mindf", (0,)),
                                 ("related_mincount", "mincount", (0,)), ("related_order", "order", ("lift",))):
                for v in bad:
                    with pytest.raises(N.NxsError) as e:
                        gidx.related(["probe"], **{kw: v})
                    assert e.value.code == INVALID and key in e.value.msg
            js = json.loads(gidx.related(["probe"], limit=2, order="share", fuzzymatch=False, json=True)[0])
            assert list(js) == ["query", "docs", "terms", "matches"] and js["query"] == "probe" and js["docs"] == 12
            assert js["terms"] == [{"term": "tie3", "count": 3, "df": 3, "score": 1.0},
                                   {"term": "tie4", "count": 3, "df": 5, "score": float(np.float32(3 / 5))}]
    finally:
        gidx.close()


# ---- 5. exclusion ---------------------------------------------------------------------------------------

@ROUTES
def test_exclusion(nxs, tmp_path, monkeypatch, route):
    rng = random.Random(5)
    words = ["linux", "lint", "unix", "erlang", "python", "kernel", "shell", "driver", "thread", "lynx"]
    docs = [(7 * i + 1, rng.sample(words, 3)) for i in range(120)]
    t, d, truth = make(tmp_path, "excl", docs)
    gidx = nxs.open_files(t, d)
    try:
        with routed(monkeypatch, gidx, route):
            got = check(gidx, truth, ["linux", "linux AND kernel", "kernel AND NOT shell", "unix OR (python AND NOT lint)"],
                        k=32, ctx="own")
            assert b"linux" not in [x[0] for x in got[0]] and not {b"kernel", b"shell"} & {x[0] for x in got[2]}
            # with related_self a single-term query's term leads "count" with c = df = n
            g = check(gidx, truth, ["linux", "kernel AND NOT shell"], k=32, include_self=True, ctx="self")
            assert g[0][0][:3] == (b"linux", g[0].docs, g[0].docs) and g[0][0][3] == 1.0
            assert b"shell" not in [x[0] for x in g[1]] and g[1][0][0] == b"kernel"     # (no doc of M holds shell)
            # a fuzzy-resolved token is excluded as the term it resolved to
            g = check(gidx, truth, ["linus", "linus AND kernel", "pythom OR shel"], k=32, fuzzymatch=True, ctx="fuzzy")
            tok = truth.ex.tokens("linus", True)
            assert len(tok) == 1 and tok[0] in [w.encode() for w in words] and tok[0] not in [x[0] for x in g[0]]
            assert g[0].docs == truth.df[tok[0]] > 0
            assert gidx.related(["linus"], fuzzymatch=False)[0].docs == 0
            # prefix and wildcard leaves: their expansions are excluded as terms
            by_df = lambda ts: sorted(ts, key=lambda w: (-truth.df[w.encode()], truth.term_ids[w.encode()]))
            for q, kw, exp in (("lin*", {"prefixmatch": True}, by_df([w for w in words if w.startswith("lin")])),
                               ("l*x AND NOT shell", {"wildcardmatch": True}, by_df([w for w in words if re.fullmatch("l.*x", w)])),
                               ("l?n* OR kernel", {"wildcardmatch": True}, by_df([w for w in words if re.fullmatch("l.n.*", w)]))):
                rw = q.replace(q.split()[0], "(" + " OR ".join(exp) + ")", 1)
                toks = [w.encode() for w in exp] + [w.encode() for w in ("shell", "kernel") if w in q]
                for order in ORDERS:
                    g = gidx.related([q], limit=32, order=order, fuzzymatch=False, **kw)[0]
                    check_related(g, truth.related(q, O.BM25, 32, order, rewritten=rw, tokens=toks), (q, order))
                    assert len(exp) >= 2 and not {w.encode() for w in exp} & {x[0] for x in g} and g.docs > 0
                g = gidx.related([q], limit=32, include_self=True, fuzzymatch=False, **kw)[0]
                check_related(g, truth.related(q, O.BM25, 32, include_self=True, rewritten=rw), (q, "self"))
    finally:
        gidx.close()


# ---- 6. snapshots ---------------------------------------------------------------------------------------

@ROUTES
def test_snapshots(nxs, tmp_path, monkeypatch, route):
    ev = [("add", 10, ["apple", "maple", "zebra"]), ("add", 20, ["apple", "apply", "pear"]),
          ("add", 30, ["ample", "apple", "pear"]), ("add", 40, ["apply", "zebra"]), ("add", 50, ["ample", "fig"]),
          ("add", 60, ["apricot", "fig"]), ("add", 70, ["kiwi", "apple"]), ("add", 80, ["lime", "kiwi"]),
          ("add", 90, ["plum", "sloe"]), ("add", 100, ["plum", "lime"]), ("rm", 60)]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 262144)
    open(d, "wb").write(dimg + b"\0" * 262144)
    gidx = nxs.open_files(t, d)
    qs = ["apple", "apple OR fig", "pear AND apple", "apple AND NOT pear", "plum OR kiwi", "sloe", "apricot", "quince OR zebra"]

    def publish(first=False):
        timg, dimg, term_ids = nxsfmt.build_images_log(ev)
        if not first:
            nxsfmt.publish_in_place(t, d, timg, dimg)
        return Truth(O.Index(t, d), [(e[1], e[2]) for e in ev if e[0] == "add"], [e[1] for e in ev if e[0] == "rm"], term_ids)

    def check_all(truth, ctx):
        for order in ORDERS:
            got = check(gidx, truth, qs, k=32, order=order, ctx=ctx)
        return got
    try:
        with routed(monkeypatch, gidx, route):
            got = check_all(publish(first=True), "snapshot 0")
            # doc 60 was removed at write time: apricot is in no live doc, and never appears
            assert got[6].docs == 0 and all(b"apricot" not in [x[0] for x in g] for g in got)
            assert (b"ample", 2, 2) in [x[:3] for x in got[1]]          # apple's doc 30 and fig's doc 50
            ev.append(("rm", 90))                                      # sloe's only doc: the term is in no doc now
            ev.append(("rm", 20))                                      # a doc of `apple`, `pear` and `apply`
            got = check_all(publish(), "removal")
            assert got[5].docs == 0 and all(b"sloe" not in [x[0] for x in g] for g in got)
            assert got[0].docs == 3 and (b"pear", 1, 1) in [x[:3] for x in got[0]]
            ev.append(("add", 130, ["apple", "quince", "zebra", "quince"]))       # a new doc with a new term
            got = check_all(publish(), "append")
            assert got[0].docs == 4 and (b"quince", 1, 1) in [x[:3] for x in got[0]] and got[7].docs == 3
    finally:
        set_route(monkeypatch, gidx, None)
        gidx.close()


# ---- 7. in flight, 8. refusals ---------------------------------------------------------------------------

@ROUTES
def test_between_begin_and_end(nxs, wide, monkeypatch, route):
    """related between search_batch_begin and _end, a fuzzy batch among those in flight: its answer and the batches'
    responses equal what they are apart"""
    t, d, truth, vocab, rare = wide
    gidx = nxs.open_files(t, d)
    b1 = ["v1 OR v2", "v3 AND v4", "probe", "v5 AND NOT v6"]
    b2 = ["v1x OR v2", "probee", "tie3 OR othr"]                     # tokens that miss the dictionary: a fuzzy pass
    mine = ["v1 AND v2", "probe", "v7 OR v8 OR v9", "prob OR tie1"]
    try:
        with routed(monkeypatch, gidx, route):
            plain1 = gidx.search_batch(b1, limit=10, fuzzymatch=False, total=True)
            plain2 = gidx.search_batch(b2, limit=10, fuzzymatch=True)
            apart = gidx.related(mine, limit=8, fuzzymatch=True)
            gidx.search_batch_begin(b1, limit=10, fuzzymatch=False, total=True)
            gidx.search_batch_begin(b2, limit=10, fuzzymatch=True)
            got = check(gidx, truth, mine, k=8, fuzzymatch=True, ctx="in flight")
            assert got == apart and [g.docs for g in got] == [g.docs for g in apart]
            r1 = gidx.search_batch_end()
            assert r1 == plain1 and [x.total for x in r1] == [x.total for x in plain1]
            assert gidx.search_batch_end() == plain2
    finally:
        gidx.close()


@ROUTES
def test_refusals(nxs, wide, tmp_path, monkeypatch, route):
    t, d, truth, vocab, rare = wide
    sh = nxs.open_shard(t, d, 0, 1)
    set_route(monkeypatch, sh, route)
    with pytest.raises(N.NxsError) as e:
        sh.related(["probe"])
    assert e.value.code == INVALID and e.value.msg == "related is not available on a doc shard"
    set_route(monkeypatch, sh, None)
    sh.close()
    # a header with fewer tokens than docs (adl < 1): BM25 scores nothing, docs 0; TF-IDF answers normally
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
    gidx, tr = nxs.open_files(tp, dp), Truth(O.Index(tp, dp), docs, (), term_ids)
    qs = ["a0", "a0 OR a1", "a1 AND NOT a2"]
    try:
        with routed(monkeypatch, gidx, route):
            got = check(gidx, tr, qs, algo="BM25", k=8, ctx="adl < 1")
            assert [(g.docs, g.matches, list(g)) for g in got] == [(0, 0, [])] * 3
            got = check(gidx, tr, qs, algo="TF-IDF", k=8, ctx="tf-idf")
            assert all(g.docs > 0 and g.matches > 0 for g in got)
    finally:
        gidx.close()


def test_an_index_that_is_never_asked_runs_no_pass(nxs, wide):
    t, d, truth, vocab, rare = wide
    gidx = nxs.open_files(t, d)
    gidx.search_batch(["v1 OR v2", "probe"], limit=10, total=True, explain=True)
    gidx.doc_terms([5000], limit=3)
    zero = {"device_queries": 0, "host_queries": 0, "passes": 0, "mask_ms": 0.0, "scan_ms": 0.0, "select_ms": 0.0,
            "merge_ms": 0.0, "calls": 0}
    assert gidx.related_profile() == zero
    gidx.related(["nosuchterm", "nosuchterm OR neitherthis"], fuzzymatch=False)     # resolves to nothing: no pass either
    assert gidx.related_profile() == zero
    gidx.set_profiling(True)
    got = gidx.related(["probe", "probe", "v1 OR v2"], limit=32, fuzzymatch=False)
    prof = gidx.related_profile(reset=True)
    assert prof["calls"] == 1 and prof["passes"] == 1 and prof["device_queries"] == 2 and prof["scan_ms"] > 0, prof
    assert prof["mask_ms"] > 0 and prof["select_ms"] > 0 and prof["merge_ms"] > 0 and got[0] == got[1]
    assert gidx.related_profile() == zero
    gidx.close()


# ---- 9. random corpora ---------------------------------------------------------------------------------

SEEDS = list(range(20))


@pytest.fixture(scope="module")
def random_corpora(tmp_path_factory):
    made = {}

    def get(seed):
        if seed not in made:
            rng = random.Random(9000 + seed)
            vocab = ["z%d" % i for i in range(rng.randint(20, 80))]
            weights = [1.0 / (i + 1) for i in range(len(vocab))]
            docs, did = [], 0
            for _ in range(rng.randint(50, 400)):
                did += rng.randint(1, 1 << 20)
                docs.append((did, rng.choices(vocab, weights, k=rng.randint(1, 5))))
            removed = [docs[i][0] for i in rng.sample(range(len(docs)), len(docs) // 10)]
            qs = [random_query(rng, vocab + ["nosuch"], 6) for _ in range(26)]
            qs += ["(%s OR %s) AND NOT (%s %s)" % tuple(rng.choices(vocab, k=4)), " OR ".join(rng.sample(vocab, 12)),
                   rng.choice(vocab) + " AND", "(" + rng.choice(vocab)]
            assert len(qs) == 30
            made[seed] = make(tmp_path_factory.mktemp("rnd%d" % seed), "rnd", docs, removed) + (qs,)
        return made[seed]
    return get


@ROUTES
@pytest.mark.parametrize("group", range(4))
def test_random_corpora(nxs, random_corpora, monkeypatch, route, group):
    """20 seeded corpora of at most 400 docs over a Zipf vocabulary of at most 80 terms, with removals; 30 random
    queries each, both orders; nothing is skipped: a query the oracle rejects is rejected with the oracle's code"""
    for seed in SEEDS[5 * group:5 * group + 5]:
        t, d, truth, qs = random_corpora(seed)
        gidx = nxs.open_files(t, d)
        fz = seed % 2 == 1
        try:
            with routed(monkeypatch, gidx, route, run=RUN if seed % 4 == 0 else None, parts=2 if seed % 3 == 0 else None):
                for order in ORDERS:
                    got = check(gidx, truth, qs, algo=("BM25", "TF-IDF")[seed % 2], k=(5, 32, 1)[seed % 3], order=order,
                                fuzzymatch=fz, mindf=1 + seed % 3, ctx=("random", seed))
                    assert isinstance(got[-2], N.NxsError)
                    assert sum(not isinstance(g, N.NxsError) and g.docs > 0 for g in got) >= 5
        finally:
            gidx.close()
