"""CPU tier for the search within a doc-id set (nxs_index_search_docs): the C-ABI surface, header text and messages,
nxs_ds_sort_unique, and nxs_ds_lane (nxs_docset.h) against a numpy brute force over random lists -- no GPU."""
import ctypes as C
import os
import random

import numpy as np

import nxsearch_amd as N

NXS_H = ["nxs_index_search_docs", "nxs_index_search_docs_batch"]
NXS_GPU_H = ["nxsgpu_search_docs", "nxsgpu_search_docs_profile"]
HOOKS = ["nxs_test_docset_sort", "nxs_test_docset_lane"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nxsearch_amd", "csrc")


def test_library_exports_the_entry_points():
    L = C.CDLL(N.LIB_PATH)
    for names, listed in ((NXS_H, N.NXS_H_SYMBOLS), (NXS_GPU_H, N.NXS_GPU_H_SYMBOLS), (HOOKS, N.NXS_HOOK_SYMBOLS)):
        for sym in names:
            assert hasattr(L, sym), sym
            assert sym in listed, sym
    for m in ("search_docs", "search_docs_profile"):
        assert callable(getattr(N.Index, m))
    hdr = open(os.path.join(ROOT, "include", "nxs.h")).read()
    for sym in NXS_H:
        assert sym + "(" in hdr, sym
    for text in ("#define\tNXS_DOCSET_MAX\t\t(1u << 22)", '"doc set too large"',
                 '"search_docs is not available for a query of more than 32 terms"',
                 '"search_docs is not available on a doc shard"', "Duplicates count once", "result_entry_cmp"):
        assert text in hdr, text
    ghdr = open(os.path.join(ROOT, "include", "nxs_gpu.h")).read()
    for text in ("nxsgpu_search_docs(", "nxsgpu_search_docs_profile(", "NXSGPU_DOCSET_PROF", "NXSGPU_DOCSET_WS", "NXSGPU_DOCSET_MAX",
                 "NXS_GPU_DOCSET=host", "NXS_GPU_DOCSET_CHUNK", "NXS_GPU_DOCSET_WS", "k_ds_ord", "k_ds_score"):
        assert text in ghdr, text
    hooks = open(os.path.join(CSRC, "nxs_hooks.h")).read()
    for sym in HOOKS:
        assert sym + "(" in hooks, sym


def sort_unique(ids):
    a = (C.c_uint64 * max(len(ids), 1))(*ids)
    n = N.lib().nxs_test_docset_sort(a, len(ids))
    return list(a[:n])


def test_sort_unique():
    rng = random.Random(22)
    assert sort_unique([]) == [] and sort_unique([7]) == [7] and sort_unique([7, 7]) == [7]
    assert sort_unique([3, 1, 2]) == [1, 2, 3]
    assert sort_unique([1, 2, 2, 3]) == [1, 2, 3]                         # ascending but not distinct: not the fast path
    assert sort_unique([5, 5, 5, 5, 1, 1]) == [1, 5]
    big = [(1 << 33) + 5, 4, (1 << 63) + 1, (1 << 32), (1 << 32) - 1, 4, (1 << 64) - 1, 0, (1 << 33) + 5]
    assert sort_unique(big) == sorted(set(big))                           # ids above 2^32 order as u64, not as their low words
    asc = sorted(rng.sample(range(1 << 40), 5000))
    assert sort_unique(asc) == asc                                        # already sorted: one pass, nothing moves
    for n in (2, 63, 64, 65, 1000):
        ids = [rng.randrange(1 << 34) if rng.random() < 0.7 else rng.randrange(50) for _ in range(n)]
        assert sort_unique(ids) == sorted(set(ids)), n
    desc = asc[::-1]
    assert sort_unique(desc) == asc
    assert sort_unique(asc[:100] + asc[:100]) == asc[:100]


# ---- nxs_ds_lane ------------------------------------------------------------------------------------------

N_DOCS = 9000           # three 4096-doc directory words


def make_lists(rng, n_terms, negative=()):
    """term id t (1 ..): a random ascending list of (doc, tf, float); the terms in `negative` score below zero in
    every third doc"""
    lists = {}
    for t in range(1, n_terms + 1):
        dens = (0.05, 0.4, 0.3, 0.002, 0.9)[t % 5]
        docs = sorted(rng.sample(range(N_DOCS), max(1, int(dens * N_DOCS))))
        if t == 1:
            docs = sorted(set(docs) | {0, 63, 64, 4095, 4096, N_DOCS - 1})      # block and word boundaries
        rows = []
        for d in docs:
            f = float(np.float32(rng.uniform(0.0, 9.0)))
            if t in negative and d % 3 == 0:
                f = -1.0
            rows.append((d, rng.randint(1, 9), f))
        lists[t] = rows
    return lists


def run_lane(plan, lists, bitmap, ords):
    """nxs_test_docset_lane for the plan's token table over `lists` -> ([hit], [score])"""
    nt = plan.n_tokens
    dt, imp, off = [], [], [0]
    for j in range(nt):
        for d, tf, f in lists.get(plan.term_id[j], []):
            dt.append((d << 32) | tf)
            imp.append(f)
        off.append(len(dt))
    n = len(ords)
    hit, score = (C.c_uint8 * max(n, 1))(), (C.c_float * max(n, 1))()
    r = N.lib().nxs_test_docset_lane((C.c_uint64 * max(len(dt), 1))(*dt), (C.c_float * max(len(imp), 1))(*imp),
                                     (C.c_uint64 * (nt + 1))(*off), nt, bitmap, N_DOCS, plan.truth, plan.prog, plan.prog_len,
                                     (C.c_uint32 * max(n, 1))(*ords), n, hit, score)
    assert r == 0
    return [bool(x) for x in hit[:n]], list(score[:n])


def brute(plan, lists, expr, words, ords):
    """the same from the definition: the expression on the words the doc holds, and the f32 sum of the non-negative
    floats in ascending token order, starting from 0"""
    maps = {t: {d: f for d, _, f in rows} for t, rows in lists.items()}
    hits, scores = [], []
    for o in ords:
        holds = {w: o in maps.get(i + 1, {}) for i, w in enumerate(words)}
        acc, scored = np.float32(0.0), False
        for j in range(plan.n_tokens):
            f = maps.get(plan.term_id[j], {}).get(o)
            if f is not None and f >= 0:
                acc = np.float32(acc + np.float32(f))
                scored = True
        hits.append(bool(expr(holds)) and scored)
        scores.append(float(acc))
    return hits, scores


def compare(plan, lists, expr, words, ctx, rng):
    ords = set(rng.sample(range(N_DOCS), 700)) | {0, 63, 64, 4095, 4096, N_DOCS - 1}
    for j in range(plan.n_tokens):                                       # and docs of every list, the sparse ones too
        ords |= {d for d, _, _ in rng.sample(lists[plan.term_id[j]], min(40, len(lists[plan.term_id[j]])))}
    ords = sorted(ords)
    want = brute(plan, lists, expr, words, ords)
    assert any(want[0]), ctx
    for bitmap in (False, True):
        hit, score = run_lane(plan, lists, bitmap, ords)
        assert hit == want[0], (ctx, bitmap)
        for o, h, s, w in zip(ords, hit, score, want[1]):
            if h:
                assert np.float32(s).tobytes() == np.float32(w).tobytes(), (ctx, bitmap, o, s, w)
    return want


def compiled(q, words):
    code, err, empty, plan = N.compile_query(q, words)
    assert code == 0 and not empty, (q, code, err)
    return plan


def test_lane_token_counts_and_shapes():
    """1, 2, 8 (truth table), 9 and 32 (postfix program) tokens; OR, AND, AND NOT, a nested expression"""
    rng = random.Random(9)
    words = ["w%d" % i for i in range(1, 41)]
    lists = make_lists(rng, 40)
    for nt in (1, 2, 8, 9, 32):
        ws = words[:nt]
        q = " OR ".join(ws)
        plan = compiled(q, words)
        assert plan.n_tokens == nt
        compare(plan, lists, lambda h, ws=ws: any(h[w] for w in ws), words, ("or", nt), rng)
        if nt >= 2:
            # the first word required, the last one forbidden, the rest optional
            q = "%s AND NOT %s" % (ws[0], ws[-1]) if nt == 2 else \
                "(%s) AND (%s) AND NOT %s" % (ws[0], " OR ".join(ws[:-1]), ws[-1])
            plan = compiled(q, words)
            assert plan.n_tokens == nt
            compare(plan, lists, lambda h, ws=ws: h[ws[0]] and not h[ws[-1]], words, ("and not", nt), rng)
    plan = compiled("(w3 OR w4) AND (w5 OR w6)", words)
    compare(plan, lists, lambda h: (h["w3"] or h["w4"]) and (h["w5"] or h["w6"]), words, "nested", rng)
    plan = compiled("w3 AND w4", words)
    compare(plan, lists, lambda h: h["w3"] and h["w4"], words, "and", rng)
    # a doc outside every list, an ordinal beyond the docs: no hit, score 0
    plan = compiled("w2 OR w3", words)
    free = [d for d in range(N_DOCS) if all(d not in {x[0] for x in lists[t]} for t in (2, 3))][:5]
    hit, score = run_lane(plan, lists, True, free + [N_DOCS, N_DOCS + 7])
    assert not any(hit) and score == [0.0] * len(hit)


def test_lane_a_term_listed_twice_adds_twice():
    """two tokens that resolved to one term (search.c:240: the token list is walked, not the term set)"""
    rng = random.Random(11)
    lists = make_lists(rng, 2)
    plan = N.GpuQuery()
    plan.n_tokens = 2
    plan.term_id[0] = plan.term_id[1] = 1
    plan.truth[0] = 0b1110                                               # t0 OR t1
    ords = [d for d, _, _ in lists[1]][:200] + [d for d in range(300) if d not in {x[0] for x in lists[1]}][:20]
    for bitmap in (False, True):
        hit, score = run_lane(plan, lists, bitmap, ords)
        fl = {d: f for d, _, f in lists[1]}
        for o, h, s in zip(ords, hit, score):
            assert h == (o in fl)
            if h:
                want = np.float32(np.float32(0.0) + np.float32(fl[o])) + np.float32(fl[o])
                assert np.float32(s).tobytes() == np.float32(want).tobytes(), (o, s, want)


def test_lane_a_negative_float_adds_nothing_and_alone_is_no_result():
    """search.c:261: rank() < 0 is skipped; a doc whose present tokens all score below zero never reaches
    nxs_resp_addresult, whatever the expression says"""
    rng = random.Random(12)
    words = ["w%d" % i for i in range(1, 5)]
    lists = make_lists(rng, 4, negative=(1, 2))
    for q, expr in (("w1", lambda h: h["w1"]), ("w1 OR w2", lambda h: h["w1"] or h["w2"]),
                    ("w1 OR w3", lambda h: h["w1"] or h["w3"]), ("w1 AND w3", lambda h: h["w1"] and h["w3"]),
                    ("w3 AND NOT w1", lambda h: h["w3"] and not h["w1"])):
        plan = compiled(q, words)
        hits, _ = compare(plan, lists, expr, words, q, rng)
    # w1 alone: exactly its docs with d % 3 != 0
    plan = compiled("w1", words)
    ords = [d for d, _, _ in lists[1]]
    hit, _ = run_lane(plan, lists, False, ords)
    assert hit == [d % 3 != 0 for d in ords] and not all(hit) and any(hit)
    assert N.lib().nxs_test_docset_lane(None, None, None, 33, False, 1, None, None, 0, None, 0, None, None) == -1
