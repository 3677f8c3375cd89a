"""GPU tier (`-m gpu`): the device index image, read back array by array (Index.device_image) and compared
with the host model of tests/index_truth.py -- on a fresh load and after each of four refreshes of one index:
removals only, appends only, a mixed one that outgrows d_post and the spare CSR buffer and moves the dense
set, and one doc with a new largest tf.  Search results never see most of this: a per-term maximum that is a
little low, a directory entry off by one, a column cell left stale.  tests/test_index_image_host.py asserts,
from the files alone, that every edge this file counts on is in the corpus.

Switches: NXS_GPU_SCANM_DENS=0.05 (df >= 1024 is then the binding dense rule at 16391 docs),
NXS_GPU_SCANS_DROP=1 (the byte columns exist), NXS_GPU_BM_SHARE=2^30 (every non-empty list has a bitmap row:
the short designed lists -- `one`, `seam`, `gap`, `late`, `run` -- are the ones with the seams)."""
import ctypes as C
import os

import numpy as np
import pytest

import index_truth as T
import nxsearch_amd as N
import nxsfmt
import oracle_lib as O

pytestmark = pytest.mark.gpu

ENV = {"NXS_GPU_SCANM_DENS": "0.05", "NXS_GPU_SCANS_DROP": "1", "NXS_GPU_BM_SHARE": str(1 << 30)}
ALGO_NAME = T.ALGO_NAME


# the checker of one image, shared with the doc-shard image tests (tests/test_docshard_image.py) and run on
# images made from the model by the CPU tier
flat_rows, check_image, canonical = T.flat_rows, T.check_image, T.canonical


class Walk:
    """One index through the five snapshots, in order; every step keeps its images and models."""

    def __init__(self, base):
        self.events, self.cut, self.ord_ids, self.info = T.corpus_events()
        self.nxs = N.Nxs(str(base))
        self.t, self.d = str(base / "nxsterms"), str(base / "nxsdtmap")
        timg, dimg, _ = nxsfmt.build_images_log(self.events[:self.cut[0]])
        # room for the appends: the files are sized once, like a preallocated index
        open(self.t, "wb").write(timg + b"\0" * (1 << 16))
        open(self.d, "wb").write(dimg + b"\0" * (1 << 18))
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

    def both_algos(self, idx):
        """one search under each ranking function: a refresh is picked up by the first, the second function's
        impacts are materialised on first use"""
        return [idx.search("all OR half", limit=10, algo=ALGO_NAME[a]) for a in (T.BM25, T.TF_IDF)]

    def step(self, k):
        ev = self.events[:self.cut[k]]
        if k:
            timg, dimg, _ = nxsfmt.build_images_log(ev)
            nxsfmt.publish_in_place(self.t, self.d, timg, dimg)
        got = self.both_algos(self.gidx)
        img = self.gidx.device_image()
        oidx = O.Index(self.t, self.d)
        # (the oracle maps the files, which the next step rewrites in place: everything is asked of it now)
        model = T.Model(ev, oidx, self.ord_ids[:T.n_ordinals(k)]).freeze()
        fresh = self.nxs.open_files(self.t, self.d)
        try:
            fgot = self.both_algos(fresh)
            fimg = fresh.device_image()
        finally:
            fresh.close()
        fmodel = T.Model(ev, oidx, T.fresh_ord_ids(ev))
        fmodel._imp, fmodel.oidx = model._imp, None     # (the same lists in the same order: the oracle is asked once)
        want = [oidx.search("all OR half", limit=10, algo=a) for a in (T.BM25, T.TF_IDF)]
        oidx.close()
        stats = (C.c_uint64 * 2)()
        L = N.lib()
        L.nxs_index_refresh_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.nxs_index_refresh_stats(self.gidx._h, stats)
        adds = [e for e in ev if e[0] == "add"]
        tf_max = lambda evs: max(max(e[2].count(t) for t in set(e[2])) for e in evs)
        live = set(T.fresh_ord_ids(ev))
        return {"img": img, "model": model, "fimg": fimg, "fmodel": fmodel, "got": got, "fgot": fgot, "want": want,
                "stats": (int(stats[0]), int(stats[1])),
                # a refresh never lowers max_tf; a fresh load sees the live docs only
                "max_tf": tf_max(adds), "fmax_tf": tf_max([e for e in adds if e[1] in live])}

    def close(self):
        self.gidx.close()
        self.nxs.close()


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    old = {k: os.environ.get(k) for k in ENV}
    os.environ.update(ENV)
    w = Walk(tmp_path_factory.mktemp("image"))
    yield w
    w.close()
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def results_same(got, want, ctx):
    assert [d for d, _ in got] == [d for d, _ in want], ctx
    assert [T.f32_bits(s) for _, s in got] == [T.f32_bits(s) for _, s in want], ctx


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_image_of_the_refreshed_index_equals_the_model(walk, k):
    """Snapshot 0 is the fresh load of the index that then takes the four refreshes (1: removals only, 2: appends
    only, 3: mixed, beyond the capacity of d_post and the spare CSR buffer, 4: a new largest tf)."""
    s = walk.upto(k)
    assert s["stats"] == (k, 0), s["stats"]            # every step an incremental refresh, never a rebuild
    for g, w, a in zip(s["got"], s["want"], ("BM25", "TF-IDF")):
        results_same(g, w, (k, a))
    seen = check_image(s["img"], s["model"], s["max_tf"], ("refreshed", k))
    names = sorted(s["model"].terms[t - 1].decode() for t in seen["dense"])
    assert names == [["all", "d1024", "d1025", "flat", "half"], ["all", "d1025", "flat", "half"],
                     ["all", "d1025", "flat", "half"], ["all", "d1023", "d1025", "flat", "half"],
                     ["all", "d1023", "d1025", "flat", "half"]][k]
    assert s["img"]["scalars"]["bm_words"] == [5, 5, 5, 6, 6][k]
    if k == 3:
        assert s["img"]["scalars"]["cap_post"] > walk.snap[2]["img"]["scalars"]["cap_post"]     # d_post moved
    if k == 4:
        assert s["img"]["scalars"]["max_tf"] > walk.snap[3]["img"]["scalars"]["max_tf"] == 200


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_image_of_a_fresh_load_equals_the_model_and_the_refreshed_index(walk, k):
    """A second index opened fresh on the same files: its whole image against the model with the fresh ordinal
    table, and canonical postings, impact bits and per-term maxima equal to the refreshed index's."""
    s = walk.upto(k)
    for g, w, a in zip(s["fgot"], s["want"], ("BM25", "TF-IDF")):
        results_same(g, w, (k, a))
    assert len(s["fmodel"].ord_ids) == s["fmodel"].n_live and s["fmodel"].live.all()
    check_image(s["fimg"], s["fmodel"], s["fmax_tf"], ("fresh", k))
    for i, (x, y) in enumerate(zip(canonical(s["img"]), canonical(s["fimg"]))):
        assert np.array_equal(x, y), (k, "fresh against refreshed", i)


def test_image_hook_refuses_batches_in_flight_and_changes_nothing(tmp_path):
    """The hook itself: an error while a batch is in flight; a part that is not materialised is empty, not an
    error; reading twice gives the same bytes and the same search results afterwards."""
    ev = [("add", i + 1, ["cat", "dog"] + ["w%d" % (i % 7)] * (1 + i % 3)) for i in range(200)]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "t"), str(tmp_path / "d")
    open(t, "wb").write(timg)
    open(d, "wb").write(dimg)
    with N.Nxs(str(tmp_path)) as nxs:
        gidx = nxs.open_files(t, d)
        before = gidx.search("cat OR w3", limit=10)
        a = gidx.device_image()
        assert a["scalars"]["algo_on"] == 2 and a["scalars"]["n_docs"] == 200
        # TF-IDF is not materialised yet, nothing is dense, the byte columns are opt-in
        for key in (("post", T.TF_IDF), ("maximp", T.TF_IDF), ("dense_col", T.BM25), ("dense_col", T.TF_IDF), "dense_terms",
                    "dense_q8", "outl_off", "outl_cap", "outl_max", "outl_post"):
            assert a[key].size == 0, key
        assert len(a[("post", T.BM25)]) == a["scalars"]["n_post"] == len(a["post_dt"])
        gidx.search_batch_begin(["cat", "dog OR w1"], limit=10)
        with pytest.raises(N.NxsError, match="in flight"):
            gidx.device_image()
        assert len(gidx.search_batch_end()) == 2
        b = gidx.device_image()
        for key in a:
            if key != "scalars":
                assert np.array_equal(a[key], b[key]), key
        assert a["scalars"] == b["scalars"]
        results_same(gidx.search("cat OR w3", limit=10), before, "after the read-back")
        gidx.search("cat", limit=10, algo="TF-IDF")
        c = gidx.device_image()
        assert c["scalars"]["algo_on"] == 3 and len(c[("post", T.TF_IDF)]) == c["scalars"]["n_post"]
        assert len(c["outl_off"]) == 1 and c["outl_post"].size == 0           # no dense term: no lists
        gidx.close()
