"""CPU tier for similar documents (nxs_index_doc_terms, nxs_index_similar): the C-ABI surface, the parameters
through the hook, the term-vector kind of nxs_sugg_t built by hand (accessors, JSON), the lookups of the shared
header nxs_docterms.h (what k_dv_scan runs per list and chunk) against a numpy brute force, and the self-removal
of nxs_index_similar on responses built by hand -- no GPU."""
import ctypes as C
import json
import os
import random
import struct

import numpy as np
import pytest

import nxsearch_amd as N
from test_explain_host import build_resp

NXS_H = ["nxs_index_doc_terms", "nxs_index_doc_terms_batch", "nxs_sugg_score", "nxs_index_similar",
         "nxs_index_similar_batch"]
NXS_GPU_H = ["nxsgpu_doc_terms", "nxsgpu_doc_terms_profile"]
HOOKS = ["nxs_test_docterms_params", "nxs_test_docterms_build", "nxs_test_docterms_lane", "nxs_test_docterms_key",
         "nxs_test_similar_drop"]
NONE = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_points():
    L = C.CDLL(N.LIB_PATH)
    for names, listed in ((NXS_H, N.NXS_H_SYMBOLS), (NXS_GPU_H, N.NXS_GPU_H_SYMBOLS), (HOOKS, N.NXS_HOOK_SYMBOLS)):
        for sym in names:
            assert hasattr(L, sym), sym
            assert sym in listed, sym
    for m in ("doc_terms", "similar", "doc_terms_profile"):
        assert callable(getattr(N.Index, m))
    hdr = open(os.path.join(ROOT, "include", "nxs.h")).read()
    for sym in NXS_H:
        assert sym + "(" in hdr, sym
    for key in ("docterms_limit", "docterms_mindf", "similar_terms", "similar_mindf", "similar_self"):
        assert '"%s"' % key in hdr, key
    ghdr = open(os.path.join(ROOT, "include", "nxs_gpu.h")).read()
    assert "nxsgpu_doc_terms(" in ghdr and "NXSGPU_DOCTERMS_PROF" in ghdr and "NXS_GPU_DOCTERMS=host" in ghdr
    hooks = open(os.path.join(ROOT, "nxsearch_amd", "csrc", "nxs_hooks.h")).read()
    for sym in HOOKS:
        assert sym + "(" in hooks, sym


def params(nxs, text):
    """-> (0, k, mindf, similar_terms, similar_mindf, similar_self) or (-1, code, message)"""
    L = N.lib()
    p = L.nxs_params_fromjson(nxs._h, text.encode(), len(text)) if text is not None else None
    assert p or text is None, text
    v = [C.c_uint(77) for _ in range(4)]
    s = C.c_int(-7)
    r = L.nxs_test_docterms_params(nxs._h, p, *[C.byref(x) for x in v], C.byref(s))
    if p:
        L.nxs_params_release(p)
    if r != 0:
        return (r,) + nxs.error()
    return (0,) + tuple(x.value for x in v) + (s.value,)


def test_params_defaults_bounds_and_names(tmp_path):
    nxs = N.Nxs(str(tmp_path))
    assert params(nxs, None) == (0, 5, 1, 8, 2, 0)
    assert params(nxs, '{"limit":3}') == (0, 5, 1, 8, 2, 0)
    assert params(nxs, '{"docterms_limit":1,"docterms_mindf":1}') == (0, 1, 1, 8, 2, 0)
    assert params(nxs, '{"docterms_limit":32,"docterms_mindf":4000000000}') == (0, 32, 4000000000, 8, 2, 0)
    assert params(nxs, '{"similar_terms":1,"similar_mindf":1,"similar_self":true}') == (0, 5, 1, 1, 1, 1)
    assert params(nxs, '{"similar_terms":32,"similar_mindf":7,"similar_self":false}') == (0, 5, 1, 32, 7, 0)
    for key, bad in (("docterms_limit", (0, 33)), ("docterms_mindf", (0,)), ("similar_terms", (0, 33)),
                     ("similar_mindf", (0,))):
        for v in bad:
            r = params(nxs, '{"%s":%d}' % (key, v))
            assert r[0] == -1 and r[1] == 3 and key in r[2], (key, v, r)
    r = params(nxs, '{"algo":"nope"}')
    assert r[0] == -1 and r[1] == 3
    nxs.close()


def build_docterms(doc, matches, rows):
    """nxs_test_docterms_build: rows [(term bytes, tf, df, score)]"""
    L = N.lib()
    n = len(rows)
    sg = L.nxs_test_docterms_build(doc, matches, n, (C.c_char_p * max(n, 1))(*[r[0] for r in rows]),
                                   (C.c_size_t * max(n, 1))(*[len(r[0]) for r in rows]),
                                   (C.c_uint * max(n, 1))(*[r[1] for r in rows]),
                                   (C.c_uint64 * max(n, 1))(*[r[2] for r in rows]),
                                   (C.c_float * max(n, 1))(*[r[3] for r in rows]))
    assert sg
    return sg


def test_the_term_vector_kind_of_the_object():
    L = N.lib()
    rows = [(b'qu"ote', 3, 12, 1.5), (b"back\\slash", 1, 1 << 33, 0.25), (b"ctl\x01\x1f", 4294967295, 2, 3.0),
            ("naïve".encode(), 2, 2, 0.0), (b"plain", 1, 1, 1e-9)]
    sg = build_docterms((1 << 40) + 5, 99, rows)
    assert L.nxs_sugg_count(sg) == 5 and L.nxs_sugg_matches(sg) == 99 and not L.nxs_sugg_dropped(sg)
    term, ln, tf, df, sc = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64(), C.c_float()
    for i, (t, wtf, wdf, w) in enumerate(rows):
        assert L.nxs_sugg_get(sg, i, C.byref(term), C.byref(ln), C.byref(tf), C.byref(df))
        assert (C.string_at(term.value, ln.value), tf.value, df.value) == (t, wtf, wdf)
        assert C.string_at(term.value, ln.value + 1)[-1:] == b"\0"
        assert L.nxs_sugg_score(sg, i, C.byref(sc)) and sc.value == C.c_float(w).value
    assert L.nxs_sugg_score(sg, 0, None)                           # the out pointer may be NULL
    assert not L.nxs_sugg_score(sg, 5, C.byref(sc)) and not L.nxs_sugg_get(sg, 5, None, None, None, None)
    n = C.c_size_t()
    text = N._take(L.nxs_sugg_tojson(sg, C.byref(n)))
    text = text if isinstance(text, str) else text.decode()
    assert n.value == len(text.encode())
    doc = json.loads(text)
    assert list(doc) == ["doc_id", "terms", "matches"] and doc["doc_id"] == (1 << 40) + 5 and doc["matches"] == 99
    assert [list(x) for x in doc["terms"]] == [["term", "tf", "df", "score"]] * 5
    assert [(x["term"].encode(), x["tf"], x["df"]) for x in doc["terms"]] == [r[:3] for r in rows]
    assert [x["score"] for x in doc["terms"]] == [C.c_float(r[3]).value for r in rows]
    assert '\\"' in text and "\\\\" in text and "\\u0001\\u001f" in text and '"score":1.5}' in text and '"score":0.0}' in text
    assert N._drain_docterms(sg) == [(t, a, b, C.c_float(w).value) for t, a, b, w in rows]    # (releases it)
    # an empty vector
    sg = build_docterms(0, 0, [])
    assert json.loads(N._take(L.nxs_sugg_tojson(sg, None))) == {"doc_id": 0, "terms": [], "matches": 0}
    L.nxs_sugg_release(sg)
    # the other kinds have no score
    L.nxs_test_sugg_build.restype = C.c_void_p
    L.nxs_test_sugg_build.argtypes = [C.c_char_p, C.c_size_t, C.c_bool, C.c_uint64, C.c_uint, C.POINTER(C.c_char_p),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_uint), C.POINTER(C.c_uint64)]
    L.nxs_test_compl_build.restype = C.c_void_p
    L.nxs_test_compl_build.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint, C.POINTER(C.c_char_p),
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    one = ((C.c_char_p * 1)(b"abc"), (C.c_size_t * 1)(3))
    for sg in (L.nxs_test_sugg_build(b"abd", 3, False, 1, 1, one[0], one[1], (C.c_uint * 1)(1), (C.c_uint64 * 1)(4)),
               L.nxs_test_compl_build(b"ab", 2, 1, 1, one[0], one[1], (C.c_uint64 * 1)(4))):
        assert sg and L.nxs_sugg_count(sg) == 1
        sc = C.c_float(-1.0)
        assert not L.nxs_sugg_score(sg, 0, C.byref(sc)) and sc.value == -1.0
        assert "score" not in str(N._take(L.nxs_sugg_tojson(sg, None)))
        L.nxs_sugg_release(sg)


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def test_the_selection_key_orders_as_the_definition_does():
    key = N.lib().nxs_test_docterms_key
    rng = random.Random(9)
    pairs = [(0.0, 1), (0.0, 2), (-0.0, 3), (1e-38, 1), (1.0, 4294967295), (1.0, 1), (3.5, 7), (3.4e38, 2)]
    pairs += [(rng.random() * 10 ** rng.randint(-5, 5), rng.randint(1, 1 << 31)) for _ in range(200)]
    keys = [key(w, t) for w, t in pairs]
    assert len(set(keys)) == len(keys) and 0 not in keys and NONE not in keys
    by_key = [p for _, p in sorted(zip(keys, pairs))]
    assert by_key == sorted(pairs, key=lambda p: (-fbits(p[0] + 0.0), p[1]))
    assert key(-0.0, 5) == key(0.0, 5)


def lane(dt, n_docs, ords, bitmap, by_posting):
    L = N.lib()
    arr = (C.c_uint64 * max(len(dt), 1))(*dt)
    o = (C.c_uint32 * max(len(ords), 1))(*ords)
    pos = (C.c_uint64 * max(len(ords), 1))()
    side = L.nxs_test_docterms_lane(arr, len(dt), bitmap, n_docs, o, len(ords), by_posting, pos)
    return side, list(pos[:len(ords)])


@pytest.mark.parametrize("n_docs", [70, 9000])
@pytest.mark.parametrize("length", [0, 1, 2, 63, 64, 65, 1000])
def test_a_list_against_a_chunk_from_either_side(length, n_docs):
    """nxs_dv_term against numpy: list lengths around the chunk size, with and without the block bitmap, chunks
    of 1 and 64 ordinals (and 2, 63), both sides forced and the kernel's own rule"""
    rng = random.Random(length * 31 + n_docs)
    length = min(length, n_docs)
    docs = np.sort(np.asarray(rng.sample(range(n_docs), length), dtype=np.uint64))
    tfs = np.asarray([rng.randint(1, 1 << 20) for _ in range(length)], dtype=np.uint64)
    dt = [int(x) for x in (docs << np.uint64(32)) | tfs]
    for nd in (1, 2, 63, 64):
        for trial in range(6):
            # ordinals that hit (list members), ordinals that miss, and the ends of the doc range
            pool = set(rng.sample(range(n_docs), min(nd, n_docs)))
            if length and trial % 2 == 0:
                pool |= set(int(x) for x in rng.sample(list(docs), min(length, nd)))
            if trial == 5:
                pool |= {0, n_docs - 1, min(4095, n_docs - 1), min(4096, n_docs - 1)}
            ords = sorted(rng.sample(sorted(pool), min(nd, len(pool))))
            at = np.searchsorted(docs, np.asarray(ords, dtype=np.uint64))
            want = [int(a) if a < length and int(docs[a]) == o else NONE for a, o in zip(at, ords)]
            for bitmap in (False, True):
                for force in (0, 1, -1):
                    side, got = lane(dt, n_docs, ords, bitmap, force)
                    assert got == want, (length, n_docs, nd, trial, bitmap, force)
                    if force >= 0:
                        assert side == force
                    else:
                        assert side == int(not bitmap and length < len(ords))
    assert N.lib().nxs_test_docterms_lane(None, 0, False, 1, None, 65, 0, None) == -1       # a chunk is 64 docs at most


def drop(results, doc, limit, total=None, tokens=None, cells=None):
    """nxs_test_similar_drop on a response built by hand -> what is left: (results, total, cells)"""
    L = N.lib()
    r = build_resp(results, total=total, tokens=tokens, cells=cells)
    try:
        L.nxs_test_similar_drop(r, doc, limit)
        out = N._drain(r, explain=tokens is not None)
        n = C.c_size_t()
        js = json.loads(N._take(L.nxs_resp_tojson(r, C.byref(n))))
        assert js["count"] == len(out) and [x["doc_id"] for x in js["results"]] == [d for d, _ in out]
        got_cells = None
        if tokens is not None:
            assert out.tokens == list(tokens)
            got_cells = out.explain
        return list(out), getattr(out, "total", None), got_cells
    finally:
        L.nxs_resp_release(r)


def test_the_self_removal_of_a_similar_search():
    toks = [b"aa", b"bb", b"cc"]
    for n in (1, 2, 5, 6):                                          # count == limit + 1 (5) and below; limit 5
        res = [(100 + 7 * i, float(50 - i)) for i in range(n)]
        cells = [[(i + 1, 0.5 + i), (0, 0.0), (i + 2, 1.5 * i + 1)] for i in range(n)]
        rows = [[(j, tf, s) for j, (tf, s) in enumerate(row) if tf] for row in cells]
        for at in list(range(n)) + [None]:                          # first / middle / last / absent
            doc = res[at][0] if at is not None else 99
            keep = [i for i in range(n) if i != at][:5]
            for total in (None, 40):
                for explained in (False, True):
                    got = drop(res, doc, 5, total=total, tokens=toks if explained else None,
                               cells=cells if explained else None)
                    ctx = (n, at, total, explained)
                    assert got[0] == [res[i] for i in keep], ctx
                    assert got[1] == (None if total is None else 39), ctx
                    assert got[2] == ([rows[i] for i in keep] if explained else None), ctx
    # the source is not among limit + 1 results: the last one goes
    res = [(i + 1, float(9 - i)) for i in range(4)]
    assert drop(res, 77, 3, total=10) == (res[:3], 9, None)
    # nothing matched (no expansion): total 0 stays 0
    assert drop([], 5, 3, total=0) == ([], 0, None)
    assert drop([], 5, 3, total=0, tokens=[], cells=[]) == ([], 0, [])
