"""CPU tier for explanations (params "explain", nxs_resp_tokens / _token / _explain): the C-ABI surface, the
parameter, the accessors and the JSON writer on responses built by hand, and the searches of the shared header
nxs_explain.h (what k_explain runs per cell) against Python's bisect -- no GPU."""
import bisect
import ctypes as C
import json
import os

import pytest

import nxsearch_amd as N

NXS_H = ["nxs_resp_tokens", "nxs_resp_token", "nxs_resp_explain"]
NXS_GPU_H = ["nxsgpu_explain", "nxsgpu_explain_profile"]
HOOKS = ["nxs_test_explain_params", "nxs_test_resp_build", "nxs_test_explain_search", "nxs_test_explain_ordinal"]
NONE = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_explain_entry_points():
    L = C.CDLL(N.LIB_PATH)
    for sym in NXS_H:
        assert hasattr(L, sym), sym
        assert sym in N.NXS_H_SYMBOLS, sym
    for sym in NXS_GPU_H:
        assert hasattr(L, sym), sym
        assert sym in N.NXS_GPU_H_SYMBOLS, sym
    for sym in HOOKS:
        assert hasattr(L, sym), sym
        assert sym in N.NXS_HOOK_SYMBOLS, sym
    assert callable(N.Index.explain_profile)
    hdr = open(os.path.join(ROOT, "include", "nxs.h")).read()
    assert '"explain": true' in hdr and "prefix_limit / explain" in hdr
    for sym in NXS_H:
        assert sym in hdr, sym
    ghdr = open(os.path.join(ROOT, "include", "nxs_gpu.h")).read()
    assert "nxsgpu_explain(" in ghdr and "NXSGPU_EXPLAIN_PROF" in ghdr


def explain_param(nxs, p):
    L = N.lib()
    L.nxs_test_explain_params.restype = C.c_int
    L.nxs_test_explain_params.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    v = C.c_int(-7)
    r = L.nxs_test_explain_params(nxs._h, p, C.byref(v))
    return r, v.value


def test_explain_param_as_a_search_reads_it(tmp_path):
    L = N.lib()
    nxs = N.Nxs(str(tmp_path))

    def parse(s):
        return L.nxs_params_fromjson(nxs._h, s.encode(), len(s))
    assert explain_param(nxs, None) == (0, 0)
    for text, want in (('{"explain":true}', 1), ('{"explain":false}', 0), ('{"limit":3}', 0),
                       ('{"limit":3,"total":true,"explain":true}', 1)):
        p = parse(text)
        assert p, text
        assert explain_param(nxs, p) == (0, want), text
        L.nxs_params_release(p)
    # a value that is not a bool behaves as a wrong-typed "fuzzymatch" / "total" does: the parse has the same
    # outcome and the search runs with the default (false)
    for val in ('"yes"', "1", "null"):
        pe, pf = parse('{"explain":%s}' % val), parse('{"total":%s}' % val)
        assert bool(pe) == bool(pf), val
        if pe:
            assert explain_param(nxs, pe) == (0, 0), val
            L.nxs_params_release(pe)
            L.nxs_params_release(pf)
    # the binding's keyword
    p = N._make_params(explain=True)
    assert p and explain_param(nxs, p) == (0, 1)
    L.nxs_params_release(p)
    assert N._make_params() is None and N._make_params(explain=False) is None
    p = N._make_params(limit=5)
    assert explain_param(nxs, p) == (0, 0)
    L.nxs_params_release(p)
    nxs.close()


def build_resp(results, total=None, tokens=None, cells=None):
    """nxs_test_resp_build: results [(id, score)], tokens [bytes] or None (not explained), cells
    [[(tf, score) per token] per result]"""
    L = N.lib()
    L.nxs_test_resp_build.restype = C.c_void_p
    L.nxs_test_resp_build.argtypes = [C.c_uint, C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.c_bool, C.c_uint64,
                                      C.c_bool, C.c_uint, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    n, m = len(results), len(tokens or [])
    ids = (C.c_uint64 * max(n, 1))(*[d for d, _ in results])
    sc = (C.c_float * max(n, 1))(*[s for _, s in results])
    terms = (C.c_char_p * max(m, 1))(*(tokens or []))
    lens = (C.c_size_t * max(m, 1))(*[len(t) for t in (tokens or [])])
    flat = [c for row in (cells or []) for c in row]
    tf = (C.c_uint32 * max(n * m, 1))(*[c[0] for c in flat])
    imp = (C.c_float * max(n * m, 1))(*[c[1] for c in flat])
    r = L.nxs_test_resp_build(n, ids, sc, total is not None, total or 0, tokens is not None, m, terms, lens, tf, imp)
    assert r
    return r


def resp_json(r):
    n = C.c_size_t()
    s = N._take(N.lib().nxs_resp_tojson(r, C.byref(n)))
    return s if isinstance(s, str) else s.decode()


def test_json_and_accessors_of_an_explained_response():
    L = N.lib()
    toks = [b"micro\"soft", b"back\\slash", b"ctl\x01\x1f", "naïve".encode(), b"plain"]
    res = [(1 << 40, 1.5), (7, 0.25), (3, 3.0)]
    cells = [[(2, 1.0), (0, 0.0), (1, 0.5), (0, 0.0), (0, 0.0)],
             [(0, 0.0), (0, 0.0), (0, 0.0), (0, 0.0), (4294967295, 0.25)],
             [(0, 0.0)] * 5]                                       # an empty "terms"
    r = build_resp(res, total=12, tokens=toks, cells=cells)
    try:
        assert L.nxs_resp_tokens(r) == 5
        term, ln = C.c_void_p(), C.c_size_t()
        for j, t in enumerate(toks):
            assert L.nxs_resp_token(r, j, C.byref(term), C.byref(ln))
            assert C.string_at(term.value, ln.value) == t
            assert C.string_at(term.value, ln.value + 1)[-1:] == b"\0"      # NUL-terminated
        assert not L.nxs_resp_token(r, 5, C.byref(term), C.byref(ln))
        assert L.nxs_resp_token(r, 0, None, None)
        sc, tf = C.c_float(), C.c_uint32()
        for i, row in enumerate(cells):
            for j, (ctf, cs) in enumerate(row):
                got = L.nxs_resp_explain(r, i, j, C.byref(sc), C.byref(tf))
                assert bool(got) == (ctf != 0), (i, j)
                if got:
                    assert (tf.value, sc.value) == (ctf, cs)
        assert L.nxs_resp_explain(r, 0, 0, None, None)              # out pointers may be NULL
        assert not L.nxs_resp_explain(r, 3, 0, C.byref(sc), C.byref(tf))
        assert not L.nxs_resp_explain(r, 0, 5, C.byref(sc), C.byref(tf))
        text = resp_json(r)
        doc = json.loads(text)
        assert doc == {
            "results": [
                {"doc_id": 1 << 40, "score": 1.5, "terms": [{"t": 0, "tf": 2, "score": 1.0}, {"t": 2, "tf": 1, "score": 0.5}]},
                {"doc_id": 7, "score": 0.25, "terms": [{"t": 4, "tf": 4294967295, "score": 0.25}]},
                {"doc_id": 3, "score": 3.0, "terms": []}],
            "count": 3, "total": 12, "tokens": [t.decode() for t in toks]}
        # escaping as nxs_sugg_tojson: '"', '\\', control bytes as \u00XX, UTF-8 passes through
        assert '"micro\\"soft"' in text and '"back\\\\slash"' in text and '"ctl\\u0001\\u001f"' in text
        assert "naïve" in text
        # member order and the reals' format (fmt_real: always a fraction digit)
        assert text.startswith('{"results":[{"doc_id":1099511627776,"score":1.5,"terms":[{"t":0,"tf":2,"score":1.0},')
        assert text.index('"count":3') < text.index('"total":12') < text.index('"tokens":[')
        # the binding's view
        out = N._drain(r, True)
        assert list(out) == res and out.total == 12 and out.tokens == toks
        assert out.explain == [[(0, 2, 1.0), (2, 1, 0.5)], [(4, 4294967295, 0.25)], []]
    finally:
        L.nxs_resp_release(r)


def test_json_without_explain_is_what_it_was():
    L = N.lib()
    r = build_resp([(5, 0.5)])
    try:
        assert resp_json(r) == '{"results":[{"doc_id":5,"score":0.5}],"count":1}'
        assert L.nxs_resp_tokens(r) == 0
        assert not L.nxs_resp_token(r, 0, None, None)
        assert not L.nxs_resp_explain(r, 0, 0, None, None)
        out = N._drain(r)
        assert out == [(5, 0.5)] and type(out) is list
    finally:
        L.nxs_resp_release(r)
    r = build_resp([(5, 0.5)], total=9)
    try:
        assert resp_json(r) == '{"results":[{"doc_id":5,"score":0.5}],"count":1,"total":9}'
    finally:
        L.nxs_resp_release(r)
    # asked, nothing matched: no tokens, and the JSON says so
    r = build_resp([], tokens=[])
    try:
        assert L.nxs_resp_tokens(r) == 0
        assert resp_json(r) == '{"results":[],"count":0,"tokens":[]}'
        out = N._drain(r, True)
        assert out == [] and out.tokens == [] and out.explain == []
    finally:
        L.nxs_resp_release(r)


# ---- the shared search header ------------------------------------------------------------------------

def header_search(docs_in_list, tfs, targets, bitmap, n_docs):
    L = N.lib()
    L.nxs_test_explain_search.restype = C.c_int
    L.nxs_test_explain_search.argtypes = [C.POINTER(C.c_uint64), C.c_uint64, C.c_bool, C.c_uint32, C.POINTER(C.c_uint32),
                                          C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    n, nd = len(docs_in_list), len(targets)
    dt = (C.c_uint64 * max(n, 1))(*[(d << 32) | t for d, t in zip(docs_in_list, tfs)])
    tg = (C.c_uint32 * max(nd, 1))(*targets)
    pos, low = (C.c_uint64 * max(nd, 1))(), (C.c_uint64 * max(nd, 1))()
    assert L.nxs_test_explain_search(dt, n, bitmap, n_docs, tg, nd, pos, low) == 0
    return list(pos)[:nd], list(low)[:nd]


def check_list(lst, n_docs, targets):
    tfs = [1 + (d * 7919) % 1000 for d in lst]
    for bitmap in (False, True):
        pos, low = header_search(lst, tfs, targets, bitmap, n_docs)
        for t, p, lo in zip(targets, pos, low):
            want_lo = bisect.bisect_left(lst, t)
            assert lo == want_lo, (len(lst), bitmap, t)
            want = want_lo if want_lo < len(lst) and lst[want_lo] == t else NONE
            assert p == want, (len(lst), bitmap, t, p, want)


LENGTHS = [0, 1, 2, 3, 63, 64, 65, 4095, 4096, 4097]


@pytest.mark.parametrize("n", LENGTHS)
def test_lower_bound_and_find_against_bisect(n):
    """Lists of every length of the issue, docs spread with gaps over 20000 ordinals (several 4096-doc words):
    the target first, last, below all, above all, in a gap, and every member and every neighbour."""
    n_docs = 20000
    lst = sorted({5 + (i * 19997) // max(n, 1) + (i % 3) for i in range(n)})
    while len(lst) < n:                                  # (the spread above may collide: fill up)
        lst = sorted(set(lst) | {lst[-1] + 2})
    lst = lst[:n]
    assert len(lst) == n and (not lst or lst[-1] < n_docs)
    targets = {0, 1, 4, n_docs - 1}
    for d in lst:
        targets.update((d - 1, d, d + 1))
    if lst:
        targets.update((lst[0], lst[-1], lst[0] - 1, lst[-1] + 1))
    check_list(lst, n_docs, sorted(t for t in targets if 0 <= t < n_docs))


@pytest.mark.parametrize("n", LENGTHS)
def test_dense_prefix_lists(n):
    """The same lengths as a run of consecutive docs from 0 (a term in every doc): no gaps below the end."""
    n_docs = max(n, 1) + 70
    lst = list(range(n))
    check_list(lst, n_docs, list(range(n_docs)))


def test_block_bit_boundaries():
    """Docs on both sides of a 64-doc block and of a 4096-doc word, alone and together; a list whose only
    postings are the last doc of one word and the first of the next; words without any posting in between."""
    n_docs = 3 * 4096 + 5
    edges = [0, 63, 64, 4095, 4096, 8191, 8192, n_docs - 1]
    every = sorted(set(e + o for e in edges for o in (-1, 0, 1) if 0 <= e + o < n_docs))
    for lst in ([63], [64], [63, 64], [4095], [4096], [4095, 4096], [0, n_docs - 1], [8192], [0, 8192],
                [63, 4096, n_docs - 1], edges, every):
        check_list(lst, n_docs, every + [100, 5000, 9000])
    # a bit set by a neighbour in the same block must not make an absent doc present
    check_list([64, 66, 127], n_docs, list(range(60, 132)))
    check_list([4094, 4097], n_docs, list(range(4090, 4100)))


def test_doc_ordinal_over_sparse_ids():
    L = N.lib()
    L.nxs_test_explain_ordinal.restype = None
    L.nxs_test_explain_ordinal.argtypes = [C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint64), C.c_size_t,
                                           C.POINTER(C.c_uint64)]
    for n in LENGTHS:
        ids = [3 + 5 * i for i in range(n)]
        if n >= 3:                                       # sparse u64 ids above 2^32 at the top
            ids[-3:] = [(1 << 32) + 7, (1 << 40) + 1, (1 << 63) + 5]
        qs = sorted(set([0, 1, 2, (1 << 32) + 6, (1 << 32) + 7, (1 << 64) - 1] + ids + [i + 1 for i in ids[:50]]
                        + [i - 1 for i in ids[-50:]]))
        a = (C.c_uint64 * max(len(ids), 1))(*ids)
        q = (C.c_uint64 * len(qs))(*qs)
        out = (C.c_uint64 * len(qs))()
        L.nxs_test_explain_ordinal(a, len(ids), q, len(qs), out)
        for x, got in zip(qs, out):
            i = bisect.bisect_left(ids, x)
            assert got == (i if i < len(ids) and ids[i] == x else NONE), (n, x)
