"""CPU tier for the total match count (params "total", nxs_resp_total): the C-ABI surface,
the parameter's parsing and the binding's keyword -- no GPU."""
import ctypes as C

import nxsearch_amd as N


def test_library_exports_the_total_entry_points():
    L = C.CDLL(N.LIB_PATH)
    for sym in ("nxs_resp_total", "nxsgpu_count", "nxsgpu_count_wide"):
        assert hasattr(L, sym), sym
        assert sym in N.NXS_H_SYMBOLS + N.NXS_GPU_H_SYMBOLS, sym
    # the device shim's carriers of a batch's totals, and the hook that reports the tile widths
    for sym in ("nxsgpu_search_totals", "nxsgpu_batch_begin_opts", "nxsgpu_batch_end_totals",
                "nxsgpu_count_tile_widths", "nxs_test_count_tile_widths"):
        assert hasattr(L, sym), sym
    w = (C.c_uint32 * 2)()
    L.nxs_test_count_tile_widths.argtypes = [C.POINTER(C.c_uint32)]
    L.nxs_test_count_tile_widths(w)
    # byte masks and word masks in the same LDS tile: four docs per word against one; the static tile
    # stays within 64 KB
    assert w[0] == 4 * w[1] and 0 < w[1] * 4 <= 65536, list(w)


def _get_bool(L, p, key):
    b = C.c_bool()
    return bool(b.value) if L.nxs_params_get_bool(p, key, C.byref(b)) == 0 else None


def test_total_param_parses_from_json(tmp_path):
    """(The params container is generic, so the parsing itself would pass without the feature; what only the
    feature adds is checked first: the accessor the key leads to, and the header that documents the key.)"""
    import os
    L = N.lib()
    assert hasattr(L, "nxs_resp_total")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nxs.h")).read()
    assert '"total": true' in hdr and "limit / algo / fuzzymatch / total" in hdr
    nxs = N.Nxs(str(tmp_path))

    def parse(s):
        return L.nxs_params_fromjson(nxs._h, s.encode(), len(s))
    p = parse('{"total":true}')
    assert p and _get_bool(L, p, b"total") is True
    L.nxs_params_release(p)
    p = parse('{"limit": 3, "total": false, "fuzzymatch": false}')
    assert p and _get_bool(L, p, b"total") is False and _get_bool(L, p, b"fuzzymatch") is False
    L.nxs_params_release(p)
    # a value of another type behaves as a wrong-typed "fuzzymatch" does: same outcome of the parse, and
    # neither is there as a bool (the search then runs with the default)
    for val in ('"yes"', "1"):
        pt, pf = parse('{"total":%s}' % val), parse('{"fuzzymatch":%s}' % val)
        assert bool(pt) == bool(pf), val
        if pt:
            assert _get_bool(L, pt, b"total") is None and _get_bool(L, pf, b"fuzzymatch") is None
            L.nxs_params_release(pt)
            L.nxs_params_release(pf)
    nxs.close()


def test_make_params_sets_the_key():
    L = N.lib()
    p = N._make_params(total=True)
    assert p and _get_bool(L, p, b"total") is True
    L.nxs_params_release(p)
    p = N._make_params(limit=5, total=True)
    u = C.c_uint64()
    assert L.nxs_params_get_uint(p, b"limit", C.byref(u)) == 0 and u.value == 5
    assert _get_bool(L, p, b"total") is True
    L.nxs_params_release(p)
    # off: nothing changes -- no params object for a default search, no key otherwise
    assert N._make_params() is None and N._make_params(total=False) is None
    p = N._make_params(limit=5)
    assert _get_bool(L, p, b"total") is None
    L.nxs_params_release(p)


def test_results_with_a_total_are_still_lists():
    r = N.Results([(7, 1.5)])
    r.total = 12
    assert r == [(7, 1.5)] and isinstance(r, list) and r.total == 12
