"""CPU tier for spelling suggestions (nxs_index_suggest): the C-ABI surface, the host ranker against
the Python truth, the parameters and the JSON writer -- no GPU."""
import ctypes as C
import json
import random

import pytest

import nxsearch_amd as N
from suggest_truth import Truth, misspell, random_words

NXS_H = ["nxs_index_suggest", "nxs_index_suggest_batch", "nxs_sugg_count", "nxs_sugg_matches", "nxs_sugg_dropped",
         "nxs_sugg_get", "nxs_sugg_tojson", "nxs_sugg_release"]
NXS_GPU_H = ["nxsgpu_suggest", "nxsgpu_suggest_profile"]
HOOKS = ["nxs_test_suggest_host", "nxs_test_suggest_params", "nxs_test_sugg_build"]


def test_library_exports_the_suggest_entry_points():
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
    assert callable(N.Index.suggest)


def host_rank(terms, dfs, token, maxdist, k):
    """nxs_test_suggest_host -> ([(id, distance, df)], matches)"""
    L = N.lib()
    n = len(terms)
    L.nxs_test_suggest_host.restype = None
    L.nxs_test_suggest_host.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                        C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32)]
    arr = host_rank.cache.get(id(terms))
    if arr is None:
        arr = ((C.c_char_p * n)(*terms), (C.c_uint32 * n)(*[len(t) for t in terms]), (C.c_uint32 * n)(*dfs))
        host_rank.cache[id(terms)] = arr
    ids, dist, df = (C.c_uint32 * k)(), (C.c_uint8 * k)(), (C.c_uint32 * k)()
    cnt, m = C.c_uint32(), C.c_uint32()
    L.nxs_test_suggest_host(arr[0], arr[1], arr[2], n, token, len(token), maxdist, k, ids, dist, df,
                            C.byref(cnt), C.byref(m))
    return [(ids[i], dist[i], df[i]) for i in range(cnt.value)], m.value


host_rank.cache = {}


def test_host_ranker_against_the_truth():
    """2000 terms over a-f, lengths 1-10, random df with zeros; 200 tokens; every k and maxdist; and a
    70-byte token between terms of 68, 69 and 72 bytes (beyond the bit-vector distance: the row DP)."""
    rng = random.Random(4711)
    terms = random_words(rng, 2000)
    long_t = bytes(rng.choice(b"abcdef") for _ in range(70))
    terms += [long_t[:68], long_t[:69], long_t + b"ab", long_t[:69] + b"f" if long_t[69:] != b"f" else long_t[:69] + b"e"]
    dfs = [rng.choice([0, 0, 1, 1, 2, 3, 5, 5, 5, 40, 1000]) for _ in terms]
    dfs[2000:] = [3, 7, 7, 0]
    truth = Truth(terms, dfs)
    tokens = [misspell(rng, rng.choice(terms[:2000])) for _ in range(196)] + [b"a", b"fe", terms[17], long_t]
    assert len(tokens) == 200
    nonempty = 0
    for k in (1, 5, 32):
        for maxdist in (1, 2):
            for tok in tokens:
                want = truth.rank(tok, k, maxdist)
                assert host_rank(terms, dfs, tok, maxdist, k) == want, (tok, k, maxdist)
                nonempty += bool(want[0])
    assert nonempty > 600
    # the long token: the 68-byte term at distance 2, the 69-byte one at 1, the 72-byte one at 2 (the dead
    # 70-byte neighbour is not eligible); equal df: the lower term id first
    assert truth.rank(long_t, 5, 2) == ([(2002, 1, 7), (2003, 2, 7), (2001, 2, 3)], 3)
    assert truth.rank(long_t, 5, 1) == ([(2002, 1, 7)], 1)
    # an exact hit comes first
    live = next(i for i in range(2000) if dfs[i] > 0)
    assert truth.rank(terms[live], 1, 2)[0] == [(live + 1, 0, dfs[live])]
    assert host_rank(terms, dfs, terms[live], 2, 1)[0] == [(live + 1, 0, dfs[live])]


@pytest.fixture()
def nxs(tmp_path):
    h = N.Nxs(str(tmp_path))
    yield h
    h.close()


def suggest_params(nxs, **kv):
    """-> (k, maxdist) as nxs_index_suggest reads the parameters, or the NxsError"""
    L = N.lib()
    L.nxs_test_suggest_params.restype = C.c_int
    L.nxs_test_suggest_params.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    p = None
    if kv:
        p = L.nxs_params_create()
        for key, v in kv.items():
            L.nxs_params_set_uint(p, key.encode(), v)
    k, md = C.c_uint(), C.c_uint()
    try:
        if L.nxs_test_suggest_params(nxs._h, p, C.byref(k), C.byref(md)) != 0:
            return N.NxsError(*nxs.error())
        return k.value, md.value
    finally:
        if p:
            L.nxs_params_release(p)


def test_parameters(nxs):
    assert suggest_params(nxs) == (5, 2)
    assert suggest_params(nxs, limit=3) == (5, 2)                  # a search's keys are not this call's
    assert suggest_params(nxs, suggest_limit=1) == (1, 2)
    assert suggest_params(nxs, suggest_limit=32, suggest_maxdist=1) == (32, 1)
    assert suggest_params(nxs, suggest_maxdist=2) == (5, 2)
    for key, bad in (("suggest_limit", 0), ("suggest_limit", 33), ("suggest_maxdist", 0), ("suggest_maxdist", 3)):
        e = suggest_params(nxs, **{key: bad})
        assert isinstance(e, N.NxsError) and e.code == 3 and key in e.msg, (key, bad, e)
    # the same through JSON params; the binding's keywords set the same keys
    L = N.lib()
    pj = b'{"suggest_limit": 7, "suggest_maxdist": 1}'
    p = L.nxs_params_fromjson(nxs._h, pj, len(pj))
    u = C.c_uint64()
    assert p and L.nxs_params_get_uint(p, b"suggest_limit", C.byref(u)) == 0 and u.value == 7
    L.nxs_params_release(p)
    assert N._suggest_params() is None
    p = N._suggest_params(limit=9, maxdist=1)
    assert L.nxs_params_get_uint(p, b"suggest_limit", C.byref(u)) == 0 and u.value == 9
    assert L.nxs_params_get_uint(p, b"suggest_maxdist", C.byref(u)) == 0 and u.value == 1
    L.nxs_params_release(p)
    assert N.ERR_NAMES[3] == "INVALID"


def build(token, rows, matches, dropped=False):
    """nxs_test_sugg_build: an nxs_sugg_t by hand"""
    L = N.lib()
    L.nxs_test_sugg_build.restype = C.c_void_p
    L.nxs_test_sugg_build.argtypes = [C.c_char_p, C.c_size_t, C.c_bool, C.c_uint64, C.c_uint, C.POINTER(C.c_char_p),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_uint), C.POINTER(C.c_uint64)]
    n = len(rows)
    sg = L.nxs_test_sugg_build(token, len(token), dropped, matches, n,
                               (C.c_char_p * max(n, 1))(*[r[0] for r in rows]),
                               (C.c_size_t * max(n, 1))(*[len(r[0]) for r in rows]),
                               (C.c_uint * max(n, 1))(*[r[1] for r in rows]),
                               (C.c_uint64 * max(n, 1))(*[r[2] for r in rows]))
    assert sg
    return sg


def test_json_of_a_hand_built_object():
    L = N.lib()
    nasty = b'q"u\\o\x01t\xc3\xa9'                                  # '"', '\', 0x01 and a two-byte character
    rows = [(nasty, 1, 12), (b"plain", 2, 1 << 40)]
    sg = build(b'to"k', rows, 7)
    # the accessors
    assert L.nxs_sugg_count(sg) == 2 and L.nxs_sugg_matches(sg) == 7 and not L.nxs_sugg_dropped(sg)
    term, ln, d, df = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64()
    assert L.nxs_sugg_get(sg, 1, C.byref(term), C.byref(ln), C.byref(d), C.byref(df))
    assert (C.string_at(term.value), ln.value, d.value, df.value) == (b"plain", 5, 2, 1 << 40)   # NUL-terminated
    assert not L.nxs_sugg_get(sg, 2, C.byref(term), C.byref(ln), C.byref(d), C.byref(df))
    assert L.nxs_sugg_get(sg, 0, None, None, None, None)
    n = C.c_size_t()
    ptr = L.nxs_sugg_tojson(sg, C.byref(n))
    raw = C.string_at(ptr, n.value)
    N._libc.free(ptr)
    want = (b'{"token":"to\\"k","suggestions":[{"term":"q\\"u\\\\o\\u0001t\xc3\xa9","distance":1,"df":12},'
            b'{"term":"plain","distance":2,"df":1099511627776}],"matches":7}')
    assert raw == want
    doc = json.loads(raw.decode("utf-8"))
    assert list(doc) == ["token", "suggestions", "matches"]
    assert [list(s) for s in doc["suggestions"]] == [["term", "distance", "df"]] * 2
    assert doc["suggestions"][0]["term"].encode("utf-8") == nasty and doc["token"] == 'to"k'
    # the binding drains the same object
    got = N._drain_sugg(sg)
    assert got == rows and got.matches == 7 and got.dropped is False and isinstance(got, list)
    # an empty list still carries its count of matches; a dropped token says so
    assert N._drain_sugg(build(b"zz", [], 0), json=True) == '{"token":"zz","suggestions":[],"matches":0}'
    got = N._drain_sugg(build(b"", [], 0, dropped=True))
    assert got == [] and got.matches == 0 and got.dropped is True
