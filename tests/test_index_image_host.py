"""CPU tier of the index image tests (no GPU): the host model of tests/index_truth.py against itself and the
oracle, its bitmap and directory on hand-made lists, the image writers of tests/nxsfmt.py against their earlier
form, and every edge the GPU tier (tests/test_index_image.py) relies on, asserted from the files alone -- a GPU
test must never pass because an edge was not there."""
import math
import random
import struct

import numpy as np
import pytest

import index_truth as T
import nxsfmt
import oracle_lib as O


# ---- the image writers: joined lists, byte for byte what the concatenating writers gave ----------------

def _old_terms_image(terms, totals):
    body = b""
    for t, tot in zip(terms, totals):
        blk = struct.pack(">H", len(t)) + t + b"\0"
        blk += b"\0" * (-len(blk) % 8)
        blk += struct.pack(">Q", tot)
        body += blk
    return nxsfmt._pad32k(b"NXS_T" + bytes([1, 0, 0]) + struct.pack(">II", len(body), 0) + body)


def _old_dtmap_image(blocks, token_count, doc_count):
    body = b""
    for doc_id, doc_len, pairs in blocks:
        body += struct.pack(">QII", doc_id, doc_len, len(pairs))
        for tid, cnt in pairs:
            body += struct.pack(">II", tid, cnt)
    return nxsfmt._pad32k(b"NXS_D" + bytes([1, 0, 0]) + struct.pack(">QQII", len(body), token_count, doc_count, 0) + body)


def _small_logs():
    """three logs the suite already writes: smoke()'s refresh, the interleaved refresh test's, the growing files'"""
    a = [("add", i + 1, ["cat", "dog", "w%d" % (i % 5)]) for i in range(40)] + [("add", 99, ["cat", "emu"])]
    rng = random.Random(97)
    vocab = ["w%d" % i for i in range(60)]
    weights = [1.0 / (i + 1) for i in range(len(vocab))]
    b = [("add", i + 1, rng.choices(vocab, weights, k=rng.randint(2, 9))) for i in range(400)]
    b += [("rm", 17), ("add", 401, ["w1", "fresh1"]), ("rm", 400), ("add", 405, ["fresh2", "fresh2", "w0"])]
    c = [("add", i + 1, ["a", "b", "c%d" % (i % 7)]) for i in range(50)] + [("rm", 50), ("rm", 1)]
    return [a, b, c]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_image_writers_are_byte_identical_to_the_concatenating_ones(which):
    ev = _small_logs()[which]
    timg, dimg, ids = nxsfmt.build_images_log(ev)
    # decode what the writer wrote and write it again the old way
    terms = sorted(ids, key=ids.get)
    n = struct.unpack_from(">I", timg, 8)[0]
    totals, at = [], 16
    while at < 16 + n:
        ln = struct.unpack_from(">H", timg, at)[0]
        at += (2 + ln + 1 + 7) // 8 * 8
        totals.append(struct.unpack_from(">Q", timg, at)[0])
        at += 8
    assert len(totals) == len(terms)
    assert timg == _old_terms_image(terms, totals)
    body, tok, docs = struct.unpack_from(">QQI", dimg, 8)
    blocks, at = [], 32
    while at < 32 + body:
        did, dl, np_ = struct.unpack_from(">QII", dimg, at)
        pairs = [struct.unpack_from(">II", dimg, at + 16 + 8 * j) for j in range(np_)]
        blocks.append((did, dl, pairs))
        at += 16 + 8 * np_
    assert len(blocks) == len(ev)
    assert dimg == _old_dtmap_image(blocks, tok, docs)
    # ... and build_images goes through the same two writers
    docs_only = [(e[1], e[2]) for e in ev if e[0] == "add"]
    removed = [e[1] for e in ev if e[0] == "rm"]
    t2, d2, _ = nxsfmt.build_images(docs_only, removed)
    assert t2 == timg and struct.unpack_from(">QQI", d2, 8) == (body, tok, docs)


# ---- bitmap and directory of hand-made lists ---------------------------------------------------------------

def _slow_bm(ordinals, words):
    bm, rk = [0] * words, []
    for o in ordinals:
        bm[o // 4096] |= 1 << ((o % 4096) // 64)
    for e in range(words + 1):
        rk.append(sum(1 for o in ordinals if o < 4096 * e))
    return bm, rk


@pytest.mark.parametrize("ordinals", [
    [], [0], [63], [64], [4095], [4096], [63, 64], [4095, 4096], [63, 64, 4095, 4096, 8191, 8192],
    [8300], list(range(4000, 4200)), [5, 12287], list(range(0, 12288, 64)), list(range(12288)),
], ids=lambda o: "n%d_%s" % (len(o), "_".join(map(str, o[:2] + o[-1:]))))
def test_model_bitmap_and_directory_on_hand_made_lists(ordinals):
    words = 3
    bm, rk = _slow_bm(ordinals, words)
    assert T.blkmap_of(ordinals, words).tolist() == bm
    assert T.bmrank_of(ordinals, words).tolist() == rk
    assert rk[0] == 0 and rk[-1] == len(ordinals)


def test_model_bitmap_seams_by_hand():
    bm = T.blkmap_of([63, 64, 4095, 4096], 2).tolist()
    assert bm == [(1 << 0) | (1 << 1) | (1 << 63), 1 << 0]
    assert T.bmrank_of([63, 64, 4095, 4096], 2).tolist() == [0, 3, 4]
    assert T.bmrank_of([], 2).tolist() == [0, 0, 0] and T.blkmap_of([], 2).tolist() == [0, 0]
    assert T.bmrank_of([4096], 2).tolist() == [0, 0, 1] and T.bmrank_of([4095], 2).tolist() == [0, 1, 1]


def test_model_outlier_cap_by_hand():
    assert T.outlier_cap([1] * 16, 8) == (None, 0)                     # nothing above the cap
    assert T.outlier_cap([1] * 14 + [2, 3], 8) == (1, 2)               # 2 <= 16 // 8
    assert T.outlier_cap([1] * 13 + [2, 2, 3], 8) == (2, 1)            # 3 above 1 is too many
    assert T.outlier_cap([70] * 16, 8) == (None, 0)                    # the clamp bin: the cap reaches 62
    assert T.outlier_cap([1] * 15 + [200], 8) == (1, 1)
    assert T.outlier_cap([61] * 8 + [62] * 8, 8) == (None, 0)          # cap 61 leaves 8 > 2 above: it runs to 62
    assert T.outlier_cap([61] * 15 + [63], 8) == (61, 1)


def test_model_dense_and_bitmap_sets_by_hand():
    dfs = {1: 1024, 2: 1023, 3: 5000, 4: 1024, 5: 0}
    assert T.dense_set(dfs, 16391, 0.05) == [1, 3, 4]
    assert T.dense_set(dfs, 16391, 0.08) == [3]                        # 0.08 x 16391 = 1311.3
    assert T.dense_set({t: 2000 + (t % 3) for t in range(1, 80)}, 16391, 0.05) == \
        sorted(sorted(range(1, 80), key=lambda t: (-(2000 + t % 3), t))[:64])
    assert T.bitmap_set(dfs, 16391, 1024) == [1, 2, 3, 4]              # df >= 16
    assert T.bitmap_set({1: 15, 2: 16}, 16391, 1024) == [2]
    assert T.bitmap_set({1: 1, 2: 0}, 16391, 1 << 30) == [1]           # never an empty row
    assert T.bitmap_set(dfs, 16391, 1024, use_blkmap=False) == []


def test_model_q8_bounds_by_hand():
    one = T.f32_bits(1.0)
    lo, hi = T.q8_bounds(np.array([one, T.f32_bits(0.5), T.f32_bits(1e-6), T.f32_bits(1 / 255.0)], dtype=np.uint32), one)
    assert lo.tolist() == [255, 128, 1, 2] and hi.tolist() == [255, 129, 2, 3]      # f32(1 / 255) > 1 / 255


# ---- the corpus of the GPU tier: the model against the oracle, and every edge the GPU tier counts on ------

@pytest.fixture(scope="module")
def snaps(tmp_path_factory):
    """the five snapshots written to files of their own, each with its oracle and the model of a refreshed index"""
    base = tmp_path_factory.mktemp("image_host")
    events, cut, ord_ids, info = T.corpus_events()
    out = []
    for k in range(5):
        timg, dimg, ids = nxsfmt.build_images_log(events[:cut[k]])
        t, d = str(base / ("t%d" % k)), str(base / ("d%d" % k))
        open(t, "wb").write(timg)
        open(d, "wb").write(dimg)
        oidx = O.Index(t, d)
        out.append({"model": T.Model(events[:cut[k]], oidx, ord_ids[:T.n_ordinals(k)]), "oidx": oidx, "ids": ids,
                    "events": events[:cut[k]]})
    return {"snaps": out, "info": info, "events": events, "cut": cut, "ord_ids": ord_ids}


def test_model_agrees_with_the_writer_and_the_oracle(snaps):
    for k, s in enumerate(snaps["snaps"]):
        m, oidx = s["model"], s["oidx"]
        assert {t: i for t, i in s["ids"].items()} == {t: i + 1 for i, t in enumerate(m.terms)}, k
        assert oidx.term_count == m.n_terms and oidx.doc_count == m.n_live, k
        assert len(m.ord_ids) == T.n_ordinals(k)
        for t in range(1, m.n_terms + 1):
            assert oidx.lookup(m.terms[t - 1]) == t, (k, t)
            assert oidx.df(t) == m.df[t], (k, m.terms[t - 1])
        # the oracle's own per-posting score is the float the one-token search returns
        for name in ("seam", "gap", "d1024"):
            t = m.tid(name)
            for algo in T.ALGOS:
                want = [T.f32_bits(oidx.score(algo, t, d)) for d, _ in m.canon[t]]
                assert m.impacts(t, algo).tolist() == want, (k, name, algo)


def test_model_tfidf_arithmetic_is_the_oracles(snaps):
    """f32(log(tf + 1)) * idf with the model's idf is, bit for bit, the oracle's TF-IDF float of every posting of
    every dense term: the expression the caps are computed with.  Where a list holds a posting with tf == cap
    (the corpus guarantees one for `all` and `half`), cap_imp is that posting's float."""
    for k, s in enumerate(snaps["snaps"]):
        m = s["model"]
        for t in m.dense_terms(len(m.ord_ids), 0.05):
            idf = T.tfidf_idf(m.n_live, m.df[t])
            want = np.array([np.float32(np.float32(math.log(int(tf) + 1)) * idf) for tf in m.tfs[t]], dtype=np.float32)
            assert m.impacts(t, T.TF_IDF).tolist() == want.view(np.uint32).tolist(), (k, m.terms[t - 1])
            cap, ords, xb, cap_bits, max_bits = m.outliers(t, 8)
            if cap is None:
                assert cap_bits == m.maximp(t, T.TF_IDF) and max_bits == 0 and not len(ords)
                continue
            at = np.flatnonzero(m.tfs[t] == cap)
            if m.terms[t - 1] in (b"all", b"half"):
                assert len(at), (k, m.terms[t - 1])
            for i in at[:3]:
                assert int(m.impacts(t, T.TF_IDF)[i]) == cap_bits, (k, m.terms[t - 1], i)
            assert len(ords) == int((m.tfs[t] > cap).sum()) and max_bits == int(xb.max())
            assert (np.diff(ords) > 0).all()


def test_model_maximp_is_the_largest_float(snaps):
    m = snaps["snaps"][0]["model"]
    for name in ("all", "half", "flat", "one", "seam", "run", "w0", "w299"):
        t = m.tid(name)
        for algo in T.ALGOS:
            vals = [T.bits_f32(int(b)) for b in m.impacts(t, algo)]
            assert T.bits_f32(m.maximp(t, algo)) == max(vals) > 0, (name, algo)
    for g in T.GHOSTS:
        assert m.maximp(m.tid(g), T.BM25) == 0 and m.maximp(m.tid(g), T.TF_IDF) == 0


def test_preconditions_of_the_gpu_corpus(snaps):
    """Everything tests/test_index_image.py counts on being there, from the files alone."""
    S = [s["model"] for s in snaps["snaps"]]
    m0 = S[0]
    name = lambda m, ts: sorted(m.terms[t - 1].decode() for t in ts)
    dense = [name(m, m.dense_terms(T.n_ordinals(k), 0.05)) for k, m in enumerate(S)]
    # snapshot 0: 4 x 4096 + 7 docs, sparse ascending ids, some above 2^32; df >= 1024 is the binding dense rule
    assert m0.n_live == 16391 == len(m0.ord_ids) and m0.live.all()
    ids = m0.ord_ids.astype(object)
    assert all(b > a for a, b in zip(ids[:-1], ids[1:])) and ids[0] > 0 and ids[-1] > 2 ** 32 > ids[0]
    assert 0.05 * T.n_ordinals(2) < 1024 <= 0.08 * 16391            # (the default density would bind instead)
    assert 1024 < 0.05 * T.n_ordinals(3) < 0.05 * T.n_ordinals(4) < 1025    # after the appends the density binds: df 1025 passes
    assert dense[0] == ["all", "d1024", "d1025", "flat", "half"]
    assert dense[1] == ["all", "d1025", "flat", "half"] == dense[2]                     # d1024 left
    assert dense[3] == ["all", "d1023", "d1025", "flat", "half"] == dense[4]            # d1023 came: columns shift
    assert S[3].tid("d1023") < S[3].tid("flat")                                         # ... that of `flat`
    assert [m0.df[m0.tid(x)] for x in ("d1023", "d1024", "d1025", "flat", "one")] == [1023, 1024, 1025, 2000, 1]
    assert S[1].df[S[1].tid("d1024")] == 1023 and S[1].df[S[1].tid("one")] == 0
    assert S[3].df[S[3].tid("d1023")] == 1025 and S[3].df[S[3].tid("d1025")] == 1025
    # the caps: 1 for `all`, 2 for `half`, none for `flat`; both lists hold a posting with tf == cap
    assert T.outlier_cap(m0.tfs[m0.tid("all")], 8)[0] == 1 and T.outlier_cap(m0.tfs[m0.tid("half")], 8)[0] == 2
    assert T.outlier_cap(m0.tfs[m0.tid("flat")], 8) == (None, 0)
    assert (m0.tfs[m0.tid("all")] == 1).any() and (m0.tfs[m0.tid("half")] == 2).any()
    # `all`: more postings than the 16384 lanes of one grid stride of k_blkmap_fill, several 4096-posting chunks
    # of the outlier kernels, the histogram's clamp bin on both sides
    tf_all = m0.tfs[m0.tid("all")]
    assert len(tf_all) == 16391 > 16384 and {40, 62, 63, 64, 200} <= set(tf_all.tolist())
    assert 16391 // 16 - 2 <= int(((tf_all >= 2) & (tf_all <= 5)).sum()) <= 16391 // 16 + 2
    th = m0.tfs[m0.tid("half")]
    assert (m0.ords[m0.tid("half")] % 2 == 0).all() and len(th) == 8196
    assert abs(int((th == 2).sum()) - len(th) // 4) <= 1 and abs(int((th == 3).sum()) - len(th) // 16) <= 1
    assert set(m0.tfs[m0.tid("flat")].tolist()) == {1}
    # the lists with designed places
    words = lambda t: sorted(set((m0.ords[t] >> 12).tolist()))
    assert words(m0.tid("gap")) == [0, 3] and words(m0.tid("late")) == [2]
    assert m0.ords[m0.tid("one")].tolist() == [16390]
    assert m0.ords[m0.tid("seam")].tolist() == [63, 64, 4095, 4096, 8191, 8192]
    run = m0.ords[m0.tid("run")]
    at = int(np.flatnonzero(run == 4000)[0])
    assert run[at:].tolist() == list(range(4000, 4200)) and 0 < at < 64 < at + 96       # the word-0 part of the
    # run crosses the end of the list's first 64-posting window; the run itself crosses the word boundary
    assert run[at + 95] == 4095 and run[at + 96] == 4096
    # three terms with adjacent ids whose only docs were removed before the first load
    g = [m0.tid(x) for x in T.GHOSTS]
    assert g == [g[0], g[0] + 1, g[0] + 2] and 1 < g[0] and g[2] < m0.n_terms
    assert [m0.df[t] for t in g] == [0, 0, 0] and m0.df[g[0] - 1] > 0 and m0.df[g[2] + 1] > 0
    assert not (set(snaps["info"]["ghost_ids"]) & set(m0.ord_ids.tolist()))
    # snapshot 1: removals only -- ordinal 0, the last ordinal (the doc of `one`), a doc inside `run`, a d1024 doc
    assert snaps["cut"][1] - snaps["cut"][0] == 4 and all(e[0] == "rm" for e in snaps["events"][snaps["cut"][0]:snaps["cut"][1]])
    dead1 = np.flatnonzero(~S[1].live).tolist()
    assert dead1 == [0, 47, 4100, 16390] and 4100 in run.tolist() and 47 in m0.ords[m0.tid("d1024")].tolist()
    assert 4000 < 4100 < 4199
    # snapshot 2: five appended docs and one new term
    ev2 = snaps["events"][snaps["cut"][1]:snaps["cut"][2]]
    assert len(ev2) == 5 and all(e[0] == "add" for e in ev2) and S[2].n_terms == S[1].n_terms + 1
    assert S[2].df[S[2].tid("newterm")] == 2
    # snapshot 3: 40 removals and 4100 appended docs; a sixth bitmap word; more postings than d_post and the
    # spare CSR buffer were sized for at the first load
    ev3 = snaps["events"][snaps["cut"][2]:snaps["cut"][3]]
    assert sum(e[0] == "rm" for e in ev3) == 40 and sum(e[0] == "add" for e in ev3) == 4100
    bm_words = [(T.n_ordinals(k) + 4095) // 4096 for k in range(5)]
    assert bm_words == [5, 5, 5, 6, 6]
    P = [sum(m.df.values()) for m in S]
    cap_post0 = P[0] + P[0] // 16 + 4096
    assert P[3] > cap_post0 and P[2] <= cap_post0, (P, cap_post0)
    assert (P[3] - P[2]) + 40 * 2 > P[2] // 16 + 4096
    assert int((~S[3].live).sum()) == 44
    # snapshot 4: one appended doc whose tf of `all` is above every earlier tf of the index
    ev4 = snaps["events"][snaps["cut"][3]:snaps["cut"][4]]
    assert len(ev4) == 1 and ev4[0][0] == "add"
    max_tf3 = max(int(tf.max()) for m in S[:4] for tf in m.tfs.values() if len(tf))
    assert max_tf3 == 200 and int(S[4].tfs[S[4].tid("all")][-1]) > max_tf3
    # appended docs carry ids above every earlier one, and no doc is added and removed within one delta
    for k in range(1, 5):
        lo, hi = snaps["cut"][k - 1], snaps["cut"][k]
        added = [e[1] for e in snaps["events"][lo:hi] if e[0] == "add"]
        before = [e[1] for e in snaps["events"][:lo] if e[0] == "add"]
        assert not added or min(added) > max(before)
        assert not (set(added) & {e[1] for e in snaps["events"][lo:hi] if e[0] == "rm"})
    # the heaviest filler stays a sparse term in every snapshot
    for m in S:
        assert max(m.df[t] for t in range(1, m.n_terms + 1) if m.terms[t - 1].startswith(b"w")) < 1024
