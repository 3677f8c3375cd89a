"""CPU tier for a query's matches listed by doc id (nxs_index_match_docs): the C-ABI surface, header text and
messages, the params keys, nxs_md_lower_bound and nxs_md_page (nxs_matchdocs.h) against a brute force, and the
nxs_docs_t accessors and JSON over objects built by hand -- no GPU."""
import ctypes as C
import json
import os
import random

import nxsearch_amd as N
from matchdocs_truth import page_of

NXS_H = ["nxs_index_match_docs", "nxs_index_match_docs_batch", "nxs_docs_count", "nxs_docs_ids", "nxs_docs_total",
         "nxs_docs_next", "nxs_docs_tojson", "nxs_docs_release"]
NXS_GPU_H = ["nxsgpu_match_docs", "nxsgpu_match_docs_profile"]
HOOKS = ["nxs_test_match_params", "nxs_test_docs_build", "nxs_test_md_lower_bound", "nxs_test_md_page"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH_MAX = 1 << 22
U64_MAX = (1 << 64) - 1
INVALID = 3


def test_library_exports_the_entry_points():
    L = C.CDLL(N.LIB_PATH)
    for names, listed in ((NXS_H, N.NXS_H_SYMBOLS), (NXS_GPU_H, N.NXS_GPU_H_SYMBOLS), (HOOKS, N.NXS_HOOK_SYMBOLS)):
        for sym in names:
            assert hasattr(L, sym), sym
            assert sym in listed, sym
    for m in ("match_docs", "match_docs_profile"):
        assert callable(getattr(N.Index, m))
    hdr = open(os.path.join(ROOT, "include", "nxs.h")).read()
    for sym in NXS_H:
        assert sym + "(" in hdr, sym
    for text in ("#define\tNXS_MATCH_MAX\t\t(1u << 22)", "typedef struct nxs_docs nxs_docs_t;", '"match_limit"', '"match_from"',
                 '{"query":"<the string as given>","docs":[1,5,9],"count":3,"total":120,"next":10}',
                 '"match_docs is not available for a query of more than 32 terms"',
                 '"match_docs is not available on a doc shard"'):
        assert text in hdr, text
    ghdr = open(os.path.join(ROOT, "include", "nxs_gpu.h")).read()
    for text in ("nxsgpu_match_docs(", "nxsgpu_match_docs_profile(", "NXSGPU_MATCHDOCS_PROF", "NXSGPU_MATCHDOCS_WS", "NXSGPU_MATCH_MAX",
                 "NXS_GPU_MATCHDOCS=host", "NXS_GPU_MATCHDOCS_RUN", "NXS_GPU_MATCHDOCS_WS", "k_md_mask", "k_md_from", "k_md_count",
                 "k_md_scan", "k_md_emit"):
        assert text in ghdr, text
    hooks = open(os.path.join(ROOT, "nxsearch_amd", "csrc", "nxs_hooks.h")).read()
    for sym in HOOKS:
        assert sym + "(" in hooks, sym


# ---- the params keys ----------------------------------------------------------------------------------------

def params(nxs, text):
    """-> (0, limit, from) or (-1, code, message)"""
    L = N.lib()
    p = L.nxs_params_fromjson(nxs._h, text.encode(), len(text)) if text is not None else None
    assert p or text is None, text
    limit, frm = C.c_uint(77), C.c_uint64(77)
    r = L.nxs_test_match_params(nxs._h, p, C.byref(limit), C.byref(frm))
    if p:
        L.nxs_params_release(p)
    if r != 0:
        return (r,) + nxs.error()
    return 0, limit.value, frm.value


def test_params_defaults_bounds_and_names(tmp_path):
    nxs = N.Nxs(str(tmp_path))
    assert params(nxs, None) == (0, 1000, 0)
    assert params(nxs, '{"limit":3,"total":true,"explain":true}') == (0, 1000, 0)
    assert params(nxs, '{"match_limit":1}') == (0, 1, 0)
    assert params(nxs, '{"match_limit":%d,"match_from":%d}' % (MATCH_MAX, U64_MAX)) == (0, MATCH_MAX, U64_MAX)
    assert params(nxs, '{"match_from":0}') == (0, 1000, 0)
    assert params(nxs, '{"match_from":4294967296}') == (0, 1000, 1 << 32)
    for v in (0, MATCH_MAX + 1, 1 << 40):
        r = params(nxs, '{"match_limit":%d}' % v)
        assert r[0] == -1 and r[1] == INVALID and "match_limit" in r[2], (v, r)
    nxs.close()


# ---- nxs_md_lower_bound, nxs_md_page ------------------------------------------------------------------------

def lower_bound(ids, frm):
    a = (C.c_uint64 * max(len(ids), 1))(*ids)
    return N.lib().nxs_test_md_lower_bound(a, len(ids), frm)


def page(member, doc_ids, frm, limit):
    """nxs_md_page over arrays at their exact sizes -> (ids, more)"""
    D = len(doc_ids)
    words = [0] * ((D + 31) // 32)
    for d in range(D):
        if member[d]:
            words[d >> 5] |= 1 << (d & 31)
    bits = (C.c_uint32 * max(len(words), 1))(*words)
    ids = (C.c_uint64 * max(D, 1))(*doc_ids)
    cap = min(limit, D)
    out = (C.c_uint64 * max(cap, 1))()
    more = C.c_bool(True)
    n = N.lib().nxs_test_md_page(bits, ids, D, frm, limit, out, C.byref(more))
    assert n <= cap
    return list(out[:n]), more.value


def test_lower_bound_against_a_brute_force():
    rng = random.Random(3)
    assert lower_bound([], 0) == 0 and lower_bound([], U64_MAX) == 0
    assert lower_bound([5], 4) == 0 and lower_bound([5], 5) == 0 and lower_bound([5], 6) == 1
    assert lower_bound([U64_MAX], U64_MAX) == 0 and lower_bound([U64_MAX - 1], U64_MAX) == 1
    for n in (1, 2, 3, 63, 64, 65, 1000):
        ids = sorted(rng.sample(range(1, 1 << 40), n - 1) + [(1 << 63) + 9])     # an id above 2^63 orders as u64
        probes = [0, ids[0] - 1, ids[0], ids[-1], ids[-1] + 1, U64_MAX] + [x + d for x in rng.sample(ids, min(n, 20)) for d in (-1, 0, 1)]
        for f in probes:
            assert lower_bound(ids, f) == sum(1 for x in ids if x < f), (n, f)


def test_page_against_a_brute_force():
    rng = random.Random(4)
    for D in (0, 1, 31, 32, 33, 64, 65, 700):
        did, doc_ids = 0, []
        for _ in range(D):
            did += rng.randint(1, 9)
            doc_ids.append(did)
        for share in (0.0, 0.1, 0.6, 1.0):
            member = [rng.random() < share for _ in range(D)]
            M = [x for x, m in zip(doc_ids, member) if m]
            froms = [0, U64_MAX] + ([doc_ids[0], doc_ids[-1], doc_ids[-1] + 1] if D else []) + \
                [x + d for x in rng.sample(doc_ids, min(D, 6)) for d in (-1, 0, 1)]
            for f in froms:
                rest = len([x for x in M if x >= f])
                for limit in sorted({1, 2, 63, 64, 65, max(rest - 1, 1), max(rest, 1), rest + 1, MATCH_MAX}):
                    ids, _, nxt = page_of(M, limit, f)
                    assert page(member, doc_ids, f, limit) == (ids, nxt is not None), (D, share, f, limit)


def test_cursor_positions_and_limits():
    """the cursor below, on, between and above ids, and at UINT64_MAX; limit 1, the remainder, the remainder +/- 1"""
    doc_ids = [10, 20, 30, 40, 50, 60]
    member = [True, False, True, True, False, True]          # M = 10, 30, 40, 60; 20 and 50 are live non-matches
    assert page(member, doc_ids, 0, 10) == ([10, 30, 40, 60], False)       # below
    assert page(member, doc_ids, 30, 10) == ([30, 40, 60], False)          # on a match: inclusive
    assert page(member, doc_ids, 20, 10) == ([30, 40, 60], False)          # on a non-match
    assert page(member, doc_ids, 31, 10) == ([40, 60], False)              # between ids
    assert page(member, doc_ids, 61, 10) == ([], False)                    # above
    assert page(member, doc_ids, U64_MAX, 10) == ([], False)
    assert page(member, doc_ids, 60, 1) == ([60], False)
    assert page(member, doc_ids, 0, 1) == ([10], True)
    assert page(member, doc_ids, 11, 3) == ([30, 40, 60], False)           # limit = the remainder
    assert page(member, doc_ids, 11, 2) == ([30, 40], True)                # the remainder - 1
    assert page(member, doc_ids, 11, 4) == ([30, 40, 60], False)           # the remainder + 1
    # a doc with id UINT64_MAX can be a match and a cursor
    assert page([True, True], [5, U64_MAX], U64_MAX, 1) == ([U64_MAX], False)
    assert page([True, True], [5, U64_MAX], 0, 1) == ([5], True)


# ---- nxs_docs_t ---------------------------------------------------------------------------------------------

def build(query, ids, total, more):
    L = N.lib()
    a = (C.c_uint64 * max(len(ids), 1))(*ids)
    d = L.nxs_test_docs_build(query, a, len(ids), total, more)
    assert d
    return d


def test_docs_object_accessors_and_json():
    L = N.lib()
    d = build(b"cat OR dog", [1, 5, 9], 120, True)
    assert L.nxs_docs_count(d) == 3 and L.nxs_docs_total(d) == 120
    assert [L.nxs_docs_ids(d)[i] for i in range(3)] == [1, 5, 9]
    nxt = C.c_uint64(77)
    assert L.nxs_docs_next(d, C.byref(nxt)) and nxt.value == 10
    n = C.c_size_t()
    text = N._take(L.nxs_docs_tojson(d, C.byref(n)))
    assert text == '{"query":"cat OR dog","docs":[1,5,9],"count":3,"total":120,"next":10}' and n.value == len(text)
    L.nxs_docs_release(d)
    # exhausted: no "next", the cursor is left alone
    d = build(b"cat", [1, 5, 9], 3, False)
    nxt = C.c_uint64(77)
    assert not L.nxs_docs_next(d, C.byref(nxt)) and nxt.value == 77
    assert N._take(L.nxs_docs_tojson(d, None)) == '{"query":"cat","docs":[1,5,9],"count":3,"total":3}'
    L.nxs_docs_release(d)
    # empty, and a page that ends one below UINT64_MAX
    d = build(b"", [], 0, False)
    assert L.nxs_docs_count(d) == 0 and N._take(L.nxs_docs_tojson(d, None)) == '{"query":"","docs":[],"count":0,"total":0}'
    L.nxs_docs_release(d)
    d = build(b"x", [U64_MAX - 1], 2, True)
    assert L.nxs_docs_next(d, C.byref(nxt)) and nxt.value == U64_MAX
    assert json.loads(N._take(L.nxs_docs_tojson(d, None))) == {"query": "x", "docs": [U64_MAX - 1], "count": 1, "total": 2,
                                                               "next": U64_MAX}
    L.nxs_docs_release(d)
    # strings escape as nxs_sugg_tojson's do
    q = 'a"b\\c\n\t\x01 é'
    d = build(q.encode(), [3], 1, False)
    text = N._take(L.nxs_docs_tojson(d, None))
    assert json.loads(text) == {"query": q, "docs": [3], "count": 1, "total": 1}
    sg = L.nxs_test_related_build(q.encode(), len(q.encode()), 0, 0, 0, None, None, None, None)
    assert sg
    stext = N._take(L.nxs_sugg_tojson(sg, None))
    L.nxs_sugg_release(sg)
    assert text.split(',"docs"')[0] == stext.split(',"docs"')[0]
    L.nxs_docs_release(d)
