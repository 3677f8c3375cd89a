"""CPU tier of the doc-shard image tests (no GPU): the shard view of the host model (index_truth.ShardModel) and
the corpus of tests/test_docshard_image.py.  From the files and the model alone, for 2 and 3 shards and every
snapshot: every edge the GPU tier counts on lies inside every shard; the appends-only snapshot really moves what
a shard with an empty share must recompute.  Then the checker itself: it accepts the image the shard model stands
for, whole, and names each of seven single wrong values."""
import numpy as np
import pytest

import index_truth as T

DENS, SHARE = T.SWITCHES[0], T.SWITCHES[1]


@pytest.fixture(scope="module")
def truth(tmp_path_factory):
    base = tmp_path_factory.mktemp("docshard_image_host")
    return {S: T.ShardTruth(base, S) for S in (2, 3)}


def _dense(m):
    return m.dense_terms(len(m.ord_ids), DENS)


def _caps(m):
    return {t: T.outlier_cap(m.tfs[t], SHARE)[0] for t in _dense(m)}


@pytest.mark.parametrize("S", [2, 3])
def test_shard_model_is_a_partition_of_the_whole_index_model(truth, S):
    """Every snapshot, refreshed and fresh tables: the shards' live docs partition the collection's, their lists
    are the whole index's lists cut by doc, in order, and the local df sum to the global one."""
    tr = truth[S]
    for k in range(T.SH_SNAPSHOTS):
        w = tr.whole[k]
        for views in (tr.shards[k], tr.fresh[k]):
            assert sorted(d for m in views for d in m.docs) == sorted(w.docs), k
            assert sum(m.n_live for m in views) == w.n_live == w.doc_count
            for t in range(1, w.n_terms + 1):
                assert sum(m.df[t] for m in views) == w.df[t], (k, t)
                for a in T.ALGOS:
                    assert sorted(np.concatenate([m.impacts(t, a) for m in views]).tolist()) == sorted(w.impacts(t, a).tolist())
            for m in views:
                assert m.df_global().tolist() == [0] + [w.df[t] for t in range(1, w.n_terms + 1)] + [0]
                assert (m.coll_live, m.coll_tokens) == (w.n_live, w.token_count)
        for m in tr.fresh[k]:
            assert m.live.all()
        # at open and after the full rebuild the refreshed collection IS a fresh one
        if k in (0, 5):
            assert [m.ord_ids.tolist() for m in tr.shards[k]] == [m.ord_ids.tolist() for m in tr.fresh[k]]
        else:
            assert [m.ord_ids.tolist() for m in tr.shards[k]] != [m.ord_ids.tolist() for m in tr.fresh[k]]


@pytest.mark.parametrize("S", [2, 3])
def test_preconditions_inside_every_shard_at_every_snapshot(truth, S):
    tr = truth[S]
    for k in range(T.SH_SNAPSHOTS):
        w, views = tr.whole[k], tr.shards[k]
        whole_rule = T.dense_set(w.df, sum(len(m.ord_ids) for m in views), DENS)
        dense = [_dense(m) for m in views]
        for s, m in enumerate(views):
            ctx, n_docs = (S, k, s), len(m.ord_ids)
            words = (n_docs + 4095) // 4096
            assert words >= 2 and DENS * n_docs < 1023, ctx         # df >= 1024 is the binding dense rule
            # list lengths 1023 / 1024 / 1025: the dense rule flips inside the shard
            by_len = {n: [t for t, df in m.df.items() if df == n] for n in (1023, 1024, 1025)}
            assert all(by_len.values()), (ctx, by_len)
            assert not set(by_len[1023]) & set(dense[s]), ctx
            assert set(by_len[1024]) <= set(dense[s]) and set(by_len[1025]) <= set(dense[s]), ctx
            # dense here and not in another shard; dense membership unlike the whole-index rule's
            assert any(t not in dense[o] for t in dense[s] for o in range(S) if o != s), ctx
            assert any((t in dense[s]) != (t in whole_rule) for t in m.df if m.df[t] > 0), ctx
            # a short list with postings at the local ordinals 63 / 64 / 4095 / 4096
            assert any(df <= 64 and {63, 64, 4095, 4096} <= set(m.ords[t].tolist()) for t, df in m.df.items()), ctx
            # an empty bitmap word in a non-empty row; empty rows side by side, inside the term range
            assert any(df > 0 and (m.blkmap(t, words) == 0).any() for t, df in m.df.items()), ctx
            assert any(m.df[t] == 0 == m.df[t + 1] and m.df[t - 1] > 0 for t in range(2, m.n_terms)), ctx
        # in at least one shard: a term the collection holds and the shard does not; every dense term with
        # local df != global df; TF-IDF caps 1, 2 and none, and a posting with tf == cap
        assert any(w.df[t] > 0 and m.df[t] == 0 for m in views for t in m.df), (S, k)
        assert any(all(m.df[t] != w.df[t] for t in _dense(m)) for m in views), (S, k)
        ok = False
        for m in views:
            caps = _caps(m)
            ok = ok or ({1, 2, None} <= set(caps.values()) and
                        all((m.tfs[t] == c).any() for t, c in caps.items() if c in (1, 2)))
        assert ok, (S, k)


@pytest.mark.parametrize("S", [2, 3])
def test_the_snapshots_are_what_the_gpu_tier_says_they_are(truth, S):
    tr = truth[S]
    delta = lambda k: tr.events[tr.cut[k - 1]:tr.cut[k]]
    kinds = lambda k: {e[0] for e in delta(k)}
    sh = tr.shards
    P = lambda k, s: sum(sh[k][s].df.values())
    last = S - 1
    # 1: removals only, every shard loses docs
    assert kinds(1) == {"rm"} and all(sh[1][s].n_live < sh[0][s].n_live for s in range(S))
    assert all(len(sh[1][s].ord_ids) == len(sh[0][s].ord_ids) for s in range(S))
    # 2: appends only: the shards before the last get an EMPTY share, yet N, the integer adl (BM25's average doc
    # length) and the term count move
    assert kinds(2) == {"add"}
    for s in range(last):
        assert sh[2][s].ord_ids.tolist() == sh[1][s].ord_ids.tolist() and sh[2][s].canon == {**sh[1][s].canon, **{
            t: [] for t in range(tr.whole[1].n_terms + 1, tr.whole[2].n_terms + 1)}}
    assert len(sh[2][last].ord_ids) == len(sh[1][last].ord_ids) + T.SH_N_APPEND2
    w1, w2 = tr.whole[1], tr.whole[2]
    assert w2.n_live > w1.n_live and w2.token_count // w2.n_live == w1.token_count // w1.n_live + 1
    assert w2.n_terms == w1.n_terms + 1
    # ... so shard 0's arrays must all move: impact bits under both functions, and at least one maximum, one
    # TF-IDF cap and one lower bound of a byte column -- a stale array could not be seen without this
    a, b = sh[1][0], sh[2][0]
    rows = range(1, w1.n_terms + 1)
    for algo in T.ALGOS:
        x, y = (np.concatenate([m.impacts(t, algo) for t in rows]) for m in (a, b))
        assert len(x) == len(y) and (x != y).mean() > 0.5, (algo, (x != y).mean())
        assert any(a.maximp(t, algo) != b.maximp(t, algo) for t in rows), algo
    assert _dense(a) == _dense(b)
    assert any(a.outliers(t, SHARE)[3] != b.outliers(t, SHARE)[3] for t in _dense(a) if _caps(a)[t] is not None)
    lows = lambda m, t: T.q8_bounds(m.impacts(t, T.BM25), m.maximp(t, T.BM25))[0]
    assert any((lows(a, t) != lows(b, t)).any() for t in _dense(a))
    # 3: mixed; more postings than the last shard's d_post (sized at open) and its spare CSR buffer hold; a new
    # term; the last shard's dense set moves; every shard loses docs
    assert kinds(3) == {"add", "rm"} and tr.whole[3].n_terms == tr.whole[2].n_terms + 1
    assert all(sh[3][s].n_live < sh[2][s].n_live for s in range(last))
    cap_post0 = P(0, last) + P(0, last) // 16 + 4096
    assert P(2, last) <= cap_post0 < P(3, last), (P(2, last), cap_post0, P(3, last))
    assert P(3, last) - P(2, last) > P(2, last) // 16 + 4096
    assert _dense(sh[3][last]) != _dense(sh[2][last])
    assert [len(m.ord_ids) for m in sh[3][:last]] == [T.SH_M] * last and len(sh[3][last].ord_ids) == T.SH_M + 5 + T.SH_N_APPEND3
    # 4: one doc with a new largest tf
    assert len(delta(4)) == 1 and kinds(4) == {"add"}
    assert tr.max_tf(4, last) > max(tr.max_tf(3, s) for s in range(S)) == 200
    # 5: one doc with an id below the highest: a full rebuild, the slices move
    (_, odd, _), = delta(5)
    assert odd < max(e[1] for e in tr.events[:tr.cut[4]] if e[0] == "add") and odd == tr.info["odd_id"]
    assert [len(m.ord_ids) for m in sh[5]] != [len(m.ord_ids) for m in sh[4]] and all(m.live.all() for m in sh[5])
    # appended docs carry ids above every earlier one; no doc is added and removed within one delta
    for k in range(1, 5):
        added = [e[1] for e in delta(k) if e[0] == "add"]
        assert not added or min(added) > max(e[1] for e in tr.events[:tr.cut[k - 1]] if e[0] == "add")
        assert not set(added) & {e[1] for e in delta(k) if e[0] == "rm"}


# ---- the checker on images made from the shard model: accepted whole, and each single wrong value named ----

@pytest.mark.parametrize("S", [2, 3])
def test_checker_accepts_the_image_the_shard_model_stands_for(truth, S):
    """Every assert of check_image is reached on a shard (dense terms with and without a cap, every bitmap row,
    df_global), at every snapshot of every shard; on a whole-index model the same image has no df_global."""
    tr = truth[S]
    for k in range(T.SH_SNAPSHOTS):
        for s, m in enumerate(tr.shards[k]):
            seen = T.check_image(T.image_of(m, tr.max_tf(k, s)), m, tr.max_tf(k, s), ("made", S, k, s))
            assert len(seen["dense"]) >= 5 and seen["bm_rows"] == sum(df > 0 for df in m.df.values())
    w = tr.whole[0]
    whole_max = T.table_max_tf(tr.events[:tr.cut[0]], w.ord_ids)
    img = T.image_of(w, whole_max)
    assert img["df_global"] is None
    T.check_image(img, w, whole_max, ("made", "whole"))
    img["df_global"] = tr.shards[0][0].df_global()
    with pytest.raises(AssertionError, match="df_global"):
        T.check_image(img, w, whole_max, ("made", "whole"))


def _stale_impact(img, tr):
    """one impact bit of shard 0 left at snapshot 1's value in snapshot 2 (its share of that refresh is empty)"""
    old, new = tr.shards[1][0], tr.shards[2][0]
    t = new.tid("all")
    at = int(img["post_off"][t]) + 77
    assert old.canon[t][77] == new.canon[t][77] and old.impacts(t, T.BM25)[77] != new.impacts(t, T.BM25)[77]
    img[("post", T.BM25)]["imp"][at] = old.impacts(t, T.BM25)[77]


def _maximp_one_ulp_low(img, tr):
    t = tr.shards[2][0].tid("half")
    img[("maximp", T.TF_IDF)][t] -= 1


def _cap_with_local_df(img, tr):
    m = tr.shards[2][0]
    c, t = next((c, t) for c, t in enumerate(_dense(m)) if _caps(m)[t] is not None)
    wrong = T.f32_bits(float(T.tfidf_cap_imp(_caps(m)[t], m.coll_live, m.df[t])))
    assert wrong != int(img["outl_cap"][c]) and m.df[t] != m.coll_df[t]
    img["outl_cap"][c] = wrong


def _q8_below_the_bound(img, tr):
    m = tr.shards[2][0]
    c = _dense(m).index(m.tid("flat"))
    o = int(m.ords[m.tid("flat")][5])
    assert img["dense_q8"][c][o] >= 2
    img["dense_q8"][c][o] -= 1


def _bmrank_off_by_one(img, tr):
    m = tr.shards[2][0]
    r = img["bm_terms"].tolist().index(m.tid("seam"))
    img["bmrank"][r * (img["scalars"]["bm_words"] + 1) + 1] += 1


def _dense_set_from_global_df(img, tr):
    m = tr.shards[2][0]
    wrong = T.dense_set(m.coll_df, len(m.ord_ids), DENS)
    assert wrong != _dense(m)
    img["dense_terms"] = np.array(wrong, dtype=np.uint32)


def _df_global_is_local(img, tr):
    m = tr.shards[2][0]
    t = m.tid("all")
    assert m.df[t] != m.coll_df[t]
    img["df_global"][t] = m.df[t]


@pytest.mark.parametrize("wrong, names_it", [
    (_stale_impact, "impact bits"), (_maximp_one_ulp_low, "maximp"), (_cap_with_local_df, "outliers"),
    (_q8_below_the_bound, "dense_q8"), (_bmrank_off_by_one, "bmrank"), (_dense_set_from_global_df, "dense_terms"),
    (_df_global_is_local, "df_global")], ids=lambda x: x.__name__.strip("_") if callable(x) else None)
def test_checker_names_a_single_wrong_value(truth, wrong, names_it):
    """Shard 0 of 2 at snapshot 2 (appends only: its share was empty).  ONE value of the image made from the model
    is changed; the assert that fails is the one of that array."""
    tr = truth[2]
    m, max_tf = tr.shards[2][0], tr.max_tf(2, 0)
    img = T.image_of(m, max_tf)
    wrong(img, tr)
    with pytest.raises(AssertionError, match=names_it):
        T.check_image(img, m, max_tf, ("made", 2, 2, 0))
