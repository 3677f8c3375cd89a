"""GPU tier (`-m gpu`): the device image of every shard of a doc-sharded collection, read back
array by array (Index.device_image) and compared with the shard view of the host model (index_truth.ShardModel)
-- at open and after each of five refreshes of one collection: removals in every shard, appends only (every
shard but the last gets an EMPTY share, yet N, adl and the collection-wide df move all its impacts, maxima,
columns and caps), a mixed one that outgrows the last shard's d_post and spare CSR buffer, one doc with a new
largest tf, and an id below the highest one, which every shard takes by a full rebuild of a new slice.

A shard scores with collection-wide statistics and keeps everything structural local; search results merged
over the shards see little of that.  tests/test_docshard_image_host.py asserts, from the files alone, that every
edge this file counts on lies inside every shard, and that the checker names a single wrong value.

Switches as in tests/test_index_image.py: NXS_GPU_SCANM_DENS=0.05 (df >= 1024 is the binding dense rule in a
shard of 8199 .. 10305 docs), NXS_GPU_SCANS_DROP=1 (the byte columns exist), NXS_GPU_BM_SHARE=2^30 (every
non-empty list has a bitmap row)."""
import ctypes as C
import os

import numpy as np
import pytest

import index_truth as T
import nxsearch_amd as N
import nxsfmt

pytestmark = pytest.mark.gpu

ENV = {"NXS_GPU_SCANM_DENS": "0.05", "NXS_GPU_SCANS_DROP": "1", "NXS_GPU_BM_SHARE": str(1 << 30)}
ALGO_NAME = T.ALGO_NAME
BOTH = (T.BM25, T.TF_IDF)       # the order of use: BM25 is the default function, TF-IDF is materialised on first use
SNAPSHOTS = list(range(T.SH_SNAPSHOTS))


def _stats(idx):
    L = N.lib()
    L.nxs_index_refresh_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 2)()
    L.nxs_index_refresh_stats(idx._h, out)
    return int(out[0]), int(out[1])


def _impact_passes(idx):
    L = N.lib()
    L.nxs_test_impact_passes.restype = C.c_uint64
    L.nxs_test_impact_passes.argtypes = [C.c_void_p]
    return int(L.nxs_test_impact_passes(idx._h))


def results_same(got, want, ctx):
    assert not isinstance(got, Exception), (ctx, got)
    assert [d for d, _ in got] == [d for d, _ in want], ctx
    assert [T.f32_bits(s) for _, s in got] == [T.f32_bits(s) for _, s in want], ctx


def images_same(a, b, ctx, keys=None):
    """part for part, the scalars included"""
    assert set(a) == set(b), ctx
    for key in keys or a:
        if key == "scalars":
            assert a[key] == b[key], (ctx, key, a[key], b[key])
        elif a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, (ctx, key)
        else:
            assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (ctx, key)


UNION_T = np.dtype([("term", "<i8"), ("doc", "<u8"), ("tf", "<i8"), ("tfidf", "<u4"), ("bm25", "<u4")])


def union(imgs):
    """the multiset over the images of (term, doc id, tf, TF-IDF impact bits, BM25 impact bits), sorted; and per
    term the largest maximum of either function"""
    parts = []
    for img in imgs:
        row, ids, tf, ti, bm = T.canonical(img)[:5]
        u = np.zeros(len(row), dtype=UNION_T)
        u["term"], u["doc"], u["tf"], u["tfidf"], u["bm25"] = row, ids, tf, ti, bm
        parts.append(u)
    u = np.sort(np.concatenate(parts), order=("term", "doc", "tf", "tfidf", "bm25"))
    return u, [np.maximum.reduce([img[("maximp", a)] for img in imgs]) for a in T.ALGOS]


class Walk:
    """One collection through the six snapshots, in order; every step keeps its images.
    form: "inproc" (nxs_docshard_refresh / nxs_docshard_search_batch on all shards), "emulated" (the rank protocol,
    the ranks played one after the other) or "rccl" (one shard of one, attached to a world-1 communicator).
    lazy: TF-IDF is first used after the refresh of snapshot 2.  beside: at every snapshot also a second collection
    and a whole index, opened fresh on the same files."""

    def __init__(self, base, truth, form, lazy=False, beside=False, n_shards=None, upto=T.SH_SNAPSHOTS - 1):
        self.tr, self.form, self.lazy, self.beside, self.last = truth, form, lazy, beside, upto
        self.S = n_shards or truth.S
        self.nxs = N.Nxs(str(base))
        self.t, self.d = str(base / "nxsterms"), str(base / "nxsdtmap")
        # the files are sized once, like a preallocated index, and published in place
        for path, k in ((self.t, 0), (self.d, 1)):
            with open(path, "wb") as f:
                f.write(truth.images[0][k] + b"\0" * (len(truth.images[upto][k]) - len(truth.images[0][k]) + 4096))
        self.shards = [self.nxs.open_shard(self.t, self.d, s, self.S) for s in range(self.S)]
        if form == "rccl":
            from nxsearch_amd import multi
            multi.attach(self.nxs, self.shards[0], 0, 1)
            self.nxs.docshard_attach(self.shards[0])
        self.snap, self.error = [], None

    def upto(self, k):
        assert k <= self.last
        if self.error is not None:
            pytest.fail("an earlier snapshot failed: %r" % (self.error,))
        while len(self.snap) <= k:
            try:
                self.snap.append(self.step(len(self.snap)))
            except BaseException as e:
                self.error = e
                raise
        return self.snap[k]

    def refresh(self):
        if self.form == "inproc":
            return self.nxs.docshard_refresh(self.shards) is True
        if self.form == "emulated":
            return self.nxs.docshard_emulated_refresh(self.shards) == [1] * self.S
        return self.nxs.docshard_refresh_rank(self.shards[0]) is True

    def search(self, shards, algo):
        """-> the result list of every rank (one, but in the emulated form)"""
        name = ALGO_NAME[algo]
        if self.form == "emulated" and shards is self.shards:
            return [r[0] for r in self.nxs.docshard_emulated_ranks(shards, [T.ShardTruth.QUERY], limit=10, algo=name)]
        if self.form == "rccl":
            return [self.nxs.docshard_search_batch_rank(shards[0], [T.ShardTruth.QUERY], limit=10, algo=name)[0]]
        return [self.nxs.docshard_search_batch(shards, [T.ShardTruth.QUERY], limit=10, algo=name)[0]]

    def step(self, k):
        before = [_impact_passes(s) for s in self.shards]
        if k:
            nxsfmt.publish_in_place(self.t, self.d, *self.tr.images[k])
            assert self.refresh(), k
            # (both forms: one impact pass per shard and refresh, whatever its share was)
        after = [_impact_passes(s) for s in self.shards]
        algos = (T.BM25,) if self.lazy and k < 2 else BOTH
        out = {"algos": algos, "got": {a: self.search(self.shards, a) for a in algos},
               "imgs": [s.device_image() for s in self.shards], "stats": [_stats(s) for s in self.shards],
               "passes": [b - a for a, b in zip(before, after)], "passes_after": [_impact_passes(s) for s in self.shards]}
        if self.beside:
            fresh = [self.nxs.open_shard(self.t, self.d, s, self.S) for s in range(self.S)]
            try:
                out["fgot"] = {a: self.search(fresh, a) for a in BOTH}
                out["fimgs"] = [s.device_image() for s in fresh]
            finally:
                for s in fresh:
                    s.close()
            whole = self.nxs.open_files(self.t, self.d)
            try:
                for a in BOTH:
                    whole.search(T.ShardTruth.QUERY, limit=10, algo=ALGO_NAME[a])
                out["wimg"] = whole.device_image()
            finally:
                whole.close()
        return out

    def close(self):
        for s in self.shards:
            s.close()
        self.nxs.close()


@pytest.fixture(scope="module")
def switches():
    old = {k: os.environ.get(k) for k in ENV}
    os.environ.update(ENV)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def truths(tmp_path_factory):
    """index_truth.ShardTruth per shard count, made on first use: files of their own, the oracle asked when each
    snapshot is written"""
    base, made = tmp_path_factory.mktemp("docshard_truth"), {}

    def get(S):
        if S not in made:
            made[S] = T.ShardTruth(base, S)
        return made[S]
    return get


@pytest.fixture(scope="module")
def walks(tmp_path_factory, switches, truths):
    made = {}
    spec = {"eager2": (2, dict(form="inproc", beside=True)), "eager3": (3, dict(form="inproc", beside=True)),
            "lazy2": (2, dict(form="inproc", lazy=True)), "emulated2": (2, dict(form="emulated")),
            "rccl": (2, dict(form="rccl", n_shards=1, upto=2))}

    def get(name):
        if name not in made:
            S, kw = spec[name]
            made[name] = Walk(tmp_path_factory.mktemp(name), truths(S), **kw)
        return made[name]
    yield get
    for w in made.values():
        w.close()


# ---- a. the refreshed collection equals the model ----------------------------------------------------------

@pytest.mark.parametrize("k", SNAPSHOTS)
@pytest.mark.parametrize("S", [2, 3])
def test_every_shard_image_of_the_refreshed_collection_equals_the_model(walks, S, k):
    w = walks("eager%d" % S)
    s, tr = w.upto(k), w.tr
    for a in BOTH:
        results_same(s["got"][a][0], tr.want[k][BOTH.index(a)], (S, k, ALGO_NAME[a]))
    for sh, img in enumerate(s["imgs"]):
        T.check_image(img, tr.shards[k][sh], tr.max_tf(k, sh), ("refreshed", S, k, sh))
        assert np.array_equal(img["df_global"], tr.shards[k][sh].df_global()), (S, k, sh)
    if 1 <= k <= 4:
        # one incremental refresh and ONE impact pass per shard -- also on the shards whose share was empty
        assert s["stats"] == [(k, 0)] * S and s["passes"] == [1] * S, (s["stats"], s["passes"])
        assert s["passes_after"] == [p + 1 for p in w.snap[k - 1]["passes_after"]]
    elif k == 5:
        assert [r for _, r in s["stats"]] == [1] * S, s["stats"]           # every shard rebuilt its slice
    if k == 3:
        last = [x["imgs"][S - 1]["scalars"]["cap_post"] for x in w.snap[:4]]
        assert last[0] == last[1] == last[2] < last[3]                      # the last shard's d_post moved
        assert all(w.snap[3]["imgs"][sh]["scalars"]["cap_post"] == w.snap[0]["imgs"][sh]["scalars"]["cap_post"] for sh in range(S - 1))
    if k == 4:
        assert s["imgs"][S - 1]["scalars"]["max_tf"] > 200 == w.snap[3]["imgs"][S - 1]["scalars"]["max_tf"]


# ---- b. the union of the shards is the whole index, without a model ---------------------------------------

@pytest.mark.parametrize("k", SNAPSHOTS)
@pytest.mark.parametrize("S", [2, 3])
def test_union_of_the_shards_is_the_whole_index(walks, S, k):
    s = walks("eager%d" % S).upto(k)
    got, got_mx = union(s["imgs"])
    want, want_mx = union([s["wimg"]])
    assert len(got) == len(want) and np.array_equal(got, want), (S, k, np.flatnonzero(got != want)[:8] if len(got) == len(want) else None)
    for a in T.ALGOS:
        assert np.array_equal(got_mx[a], want_mx[a]), (S, k, ALGO_NAME[a], "the largest maximum over the shards")


# ---- c. a collection opened fresh on the same files -------------------------------------------------------

@pytest.mark.parametrize("k", SNAPSHOTS)
@pytest.mark.parametrize("S", [2, 3])
def test_every_shard_image_of_a_fresh_collection_equals_the_model_and_the_refreshed_union(walks, S, k):
    w = walks("eager%d" % S)
    s, tr = w.upto(k), w.tr
    for a in BOTH:
        results_same(s["fgot"][a][0], tr.want[k][BOTH.index(a)], (S, k, ALGO_NAME[a]))
    for sh, img in enumerate(s["fimgs"]):
        T.check_image(img, tr.fresh[k][sh], tr.max_tf(k, sh, fresh=True), ("fresh", S, k, sh))
    (got, got_mx), (want, want_mx) = union(s["fimgs"]), union(s["imgs"])
    assert np.array_equal(got, want), (S, k)
    assert all(np.array_equal(got_mx[a], want_mx[a]) for a in T.ALGOS), (S, k)
    if k == 5:
        # after the full rebuild the refreshed shards ARE freshly opened ones: array for array, ordinals included
        for sh in range(S):
            images_same(s["imgs"][sh], s["fimgs"][sh], ("rebuilt against fresh", S, sh))


# ---- d. the second ranking function, materialised after set_global_df and two refreshes --------------------

@pytest.mark.parametrize("k", SNAPSHOTS)
def test_tfidf_first_used_after_the_appends_only_refresh(walks, k):
    w, e = walks("lazy2"), walks("eager2")
    s, ref = w.upto(k), e.upto(k)
    assert s["algos"] == ((T.BM25,) if k < 2 else BOTH)
    for sh, img in enumerate(s["imgs"]):
        # (absent parts: check_image asserts need == 0 for every part of a function that is not materialised)
        T.check_image(img, w.tr.shards[k][sh], w.tr.max_tf(k, sh), ("lazy", k, sh), algos=s["algos"])
        if k < 2:
            for key in (("post", T.TF_IDF), ("maximp", T.TF_IDF), ("dense_col", T.TF_IDF), "outl_off", "outl_cap", "outl_max", "outl_post"):
                assert img[key].size == 0, (k, sh, key)
            same = [key for key in img if key != "scalars" and not (isinstance(key, tuple) and key[1] == T.TF_IDF)
                    and not str(key).startswith("outl_")]
            images_same(img, ref["imgs"][sh], ("lazy against eager", k, sh), keys=same)
        else:
            images_same(img, ref["imgs"][sh], ("lazy against eager", k, sh))
    for a in s["algos"]:
        results_same(s["got"][a][0], w.tr.want[k][BOTH.index(a)], ("lazy", k, ALGO_NAME[a]))


# ---- e. the rank form ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", SNAPSHOTS)
def test_rank_form_emulated_fills_the_same_images(walks, k):
    w, e = walks("emulated2"), walks("eager2")
    s, ref = w.upto(k), e.upto(k)
    for a in BOTH:
        for rank, got in enumerate(s["got"][a]):
            results_same(got, w.tr.want[k][BOTH.index(a)], ("emulated", k, rank, ALGO_NAME[a]))
    for sh in range(2):
        images_same(s["imgs"][sh], ref["imgs"][sh], ("emulated against in-process", k, sh))


def test_rank_form_attached_to_a_world_of_one(walks):
    """nxs_docshard_attach / nxs_docshard_refresh_rank on a real communicator of one rank, snapshots 0 .. 2: one
    shard holds the collection, its df_global is its local df, and the image is the model's."""
    w = walks("rccl")
    tr = w.tr
    tables = T.shard_ord_tables(tr.events, tr.cut[:3], 1)
    for k in range(3):
        s = w.upto(k)
        m = T.ShardModel(tr.whole[k], tables[k][0][0])
        for a in BOTH:
            results_same(s["got"][a][0], tr.want[k][BOTH.index(a)], ("rccl", k, ALGO_NAME[a]))
        T.check_image(s["imgs"][0], m, T.table_max_tf(tr.events[:tr.cut[k]], tables[k][0][0]), ("rccl", k))
        local = np.array([0] + [m.df[t] for t in range(1, m.n_terms + 1)] + [0], dtype=np.uint32)
        assert np.array_equal(s["imgs"][0]["df_global"], local), k
        if k:
            assert s["stats"] == [(k, 0)] and s["passes"] == [1]


# ---- f. the hook's new part ---------------------------------------------------------------------------------

def test_df_global_part_of_the_hook(tmp_path):
    """None on an index that is no shard; refused while a batch is in flight; read twice: the same bytes."""
    ev = [("add", i + 1, ["cat", "dog"] + ["w%d" % (i % 7)] * (1 + i % 3)) for i in range(200)]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "t"), str(tmp_path / "d")
    open(t, "wb").write(timg)
    open(d, "wb").write(dimg)
    with N.Nxs(str(tmp_path)) as nxs:
        whole = nxs.open_files(t, d)
        whole.search("cat", limit=10)
        assert whole.device_image()["df_global"] is None
        whole.close()
        shards = [nxs.open_shard(t, d, s, 2) for s in range(2)]
        assert all(s.device_image()["df_global"] is None for s in shards)      # (not set before the first search)
        nxs.docshard_search_batch(shards, ["cat OR w3"], limit=10)
        a = [s.device_image() for s in shards]
        # 200 docs of `cat`, 100 in either shard
        assert all(len(x["df_global"]) == x["scalars"]["n_terms"] + 2 and x["df_global"][1] == 200 for x in a)
        assert all(x["post_off"][2] - x["post_off"][1] == 100 for x in a)
        shards[0].search_batch_begin(["cat", "dog OR w1"], limit=10)
        with pytest.raises(N.NxsError, match="in flight"):
            shards[0].device_image()
        assert len(shards[0].search_batch_end()) == 2
        for x, s in zip(a, shards):
            images_same(x, s.device_image(), "read twice")
        for s in shards:
            s.close()
