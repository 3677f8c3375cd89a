"""CPU tier for related terms (nxs_index_related): the C-ABI surface and header text, the parameters through the
hook, the related kind of nxs_sugg_t built by hand (accessors, nxs_sugg_docs, JSON), and nxs_related.h's key,
share, predicate and host ranker against a numpy brute force -- no GPU."""
import ctypes as C
import json
import os
import random
import struct

import numpy as np

import nxsearch_amd as N

NXS_H = ["nxs_index_related", "nxs_index_related_batch", "nxs_sugg_docs"]
NXS_GPU_H = ["nxsgpu_related", "nxsgpu_related_profile"]
HOOKS = ["nxs_test_related_params", "nxs_test_related_build", "nxs_test_related_key", "nxs_test_related_share",
         "nxs_test_related_eligible", "nxs_test_related_rank"]
KEYS = ("related_limit", "related_order", "related_mindf", "related_mincount", "related_self")
NONE = (1 << 64) - 1
COUNT, SHARE = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_points():
    L = C.CDLL(N.LIB_PATH)
    for names, listed in ((NXS_H, N.NXS_H_SYMBOLS), (NXS_GPU_H, N.NXS_GPU_H_SYMBOLS), (HOOKS, N.NXS_HOOK_SYMBOLS)):
        for sym in names:
            assert hasattr(L, sym), sym
            assert sym in listed, sym
    for m in ("related", "related_profile"):
        assert callable(getattr(N.Index, m))
    hdr = open(os.path.join(ROOT, "include", "nxs.h")).read()
    for sym in NXS_H:
        assert sym + "(" in hdr, sym
    for key in KEYS:
        assert '"%s"' % key in hdr, key
    assert '{"query":"<the string as given>","docs":n,"terms":[{"term":"...","count":c,"df":df,"score":s},...],"matches":M}' in hdr
    assert "related is not available on a doc shard" in hdr
    ghdr = open(os.path.join(ROOT, "include", "nxs_gpu.h")).read()
    for text in ("nxsgpu_related(", "nxsgpu_related_profile(", "NXSGPU_RELATED_PROF", "NXSGPU_RELATED_WS", "NXS_GPU_RELATED=host",
                 "NXS_GPU_RELATED_RUN", "NXS_GPU_RELATED_PARTS", "NXS_GPU_RELATED_WS", "k_rt_mask", "k_rt_scan", "k_rt_select"):
        assert text in ghdr, text
    hooks = open(os.path.join(ROOT, "nxsearch_amd", "csrc", "nxs_hooks.h")).read()
    for sym in HOOKS:
        assert sym + "(" in hooks, sym


def params(nxs, text):
    """-> (0, k, order, mindf, mincount, self) or (-1, code, message)"""
    L = N.lib()
    p = L.nxs_params_fromjson(nxs._h, text.encode(), len(text)) if text is not None else None
    assert p or text is None, text
    k, mindf, mincount = C.c_uint(77), C.c_uint(77), C.c_uint(77)
    order, self_ = C.c_int(-7), C.c_int(-7)
    r = L.nxs_test_related_params(nxs._h, p, C.byref(k), C.byref(order), C.byref(mindf), C.byref(mincount), C.byref(self_))
    if p:
        L.nxs_params_release(p)
    if r != 0:
        return (r,) + nxs.error()
    return 0, k.value, order.value, mindf.value, mincount.value, self_.value


def test_params_defaults_bounds_and_names(tmp_path):
    nxs = N.Nxs(str(tmp_path))
    assert params(nxs, None) == (0, 5, COUNT, 1, 1, 0)
    assert params(nxs, '{"limit":3,"total":true,"explain":true}') == (0, 5, COUNT, 1, 1, 0)
    assert params(nxs, '{"related_limit":1,"related_mindf":1,"related_mincount":1}') == (0, 1, COUNT, 1, 1, 0)
    assert params(nxs, '{"related_limit":32,"related_mindf":4294967295,"related_mincount":4000000000}') == \
        (0, 32, COUNT, 4294967295, 4000000000, 0)
    assert params(nxs, '{"related_order":"share","related_self":true}') == (0, 5, SHARE, 1, 1, 1)
    assert params(nxs, '{"related_order":"count","related_self":false}') == (0, 5, COUNT, 1, 1, 0)
    for key, bad in (("related_limit", (0, 33, 1 << 40)), ("related_mindf", (0, 1 << 32)), ("related_mincount", (0, 1 << 32))):
        for v in bad:
            r = params(nxs, '{"%s":%d}' % (key, v))
            assert r[0] == -1 and r[1] == 3 and key in r[2], (key, v, r)
    for bad in ("lift", "", "Count", "share "):
        r = params(nxs, '{"related_order":"%s"}' % bad)
        assert r[0] == -1 and r[1] == 3 and "related_order" in r[2], (bad, r)
    nxs.close()


def build_related(query, docs, matches, rows):
    """nxs_test_related_build: rows [(term bytes, c, df)]"""
    L = N.lib()
    n = len(rows)
    sg = L.nxs_test_related_build(query, len(query), docs, matches, n, (C.c_char_p * max(n, 1))(*[r[0] for r in rows]),
                                  (C.c_size_t * max(n, 1))(*[len(r[0]) for r in rows]),
                                  (C.c_uint * max(n, 1))(*[r[1] for r in rows]),
                                  (C.c_uint64 * max(n, 1))(*[r[2] for r in rows]))
    assert sg
    return sg


def f32(x):
    return float(np.float32(x))


def test_the_related_kind_of_the_object():
    L = N.lib()
    query = b'say "hi" \\ AND ctl\x01 OR na\xc3\xafve'
    rows = [(b'qu"ote', 3, 12), (b"back\\slash", 1, 4000000000), (b"ctl\x01\x1f", 4294967295, 4294967295),
            ("naïve".encode(), 2, 3), (b"plain", 1, 1)]
    sg = build_related(query, (1 << 33) + 9, 99, rows)
    assert L.nxs_sugg_count(sg) == 5 and L.nxs_sugg_matches(sg) == 99 and not L.nxs_sugg_dropped(sg)
    docs = C.c_uint64(0)
    assert L.nxs_sugg_docs(sg, C.byref(docs)) and docs.value == (1 << 33) + 9 and L.nxs_sugg_docs(sg, None)
    term, ln, c, df, sc = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64(), C.c_float()
    for i, (t, wc, wdf) in enumerate(rows):
        assert L.nxs_sugg_get(sg, i, C.byref(term), C.byref(ln), C.byref(c), C.byref(df))
        assert (C.string_at(term.value, ln.value), c.value, df.value) == (t, wc, wdf)
        assert L.nxs_sugg_score(sg, i, C.byref(sc)) and sc.value == f32(wc / wdf)
    assert not L.nxs_sugg_score(sg, 5, C.byref(sc)) and not L.nxs_sugg_get(sg, 5, None, None, None, None)
    n = C.c_size_t()
    text = N._take(L.nxs_sugg_tojson(sg, C.byref(n)))
    text = text if isinstance(text, str) else text.decode()
    assert n.value == len(text.encode())
    doc = json.loads(text)
    assert list(doc) == ["query", "docs", "terms", "matches"]
    assert doc["query"].encode() == query and doc["docs"] == (1 << 33) + 9 and doc["matches"] == 99
    assert [list(x) for x in doc["terms"]] == [["term", "count", "df", "score"]] * 5
    assert [(x["term"].encode(), x["count"], x["df"]) for x in doc["terms"]] == rows
    assert [x["score"] for x in doc["terms"]] == [f32(r[1] / r[2]) for r in rows]
    assert '\\"' in text and "\\\\" in text and "\\u0001\\u001f" in text and '"score":0.25}' in text and '"score":1.0}' in text
    got = N._drain_related(sg)                                      # (releases it)
    assert got == [(t, a, b, f32(a / b)) for t, a, b in rows] and got.matches == 99 and got.docs == (1 << 33) + 9
    # an empty list
    sg = build_related(b"", 0, 0, [])
    assert json.loads(N._take(L.nxs_sugg_tojson(sg, None))) == {"query": "", "docs": 0, "terms": [], "matches": 0}
    L.nxs_sugg_release(sg)


def test_the_other_kinds_report_no_docs():
    L = N.lib()
    L.nxs_test_sugg_build.restype = C.c_void_p
    L.nxs_test_sugg_build.argtypes = [C.c_char_p, C.c_size_t, C.c_bool, C.c_uint64, C.c_uint, C.POINTER(C.c_char_p),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_uint), C.POINTER(C.c_uint64)]
    L.nxs_test_compl_build.restype = C.c_void_p
    L.nxs_test_compl_build.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint, C.POINTER(C.c_char_p),
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    L.nxs_test_wild_build.restype = C.c_void_p
    L.nxs_test_wild_build.argtypes = L.nxs_test_compl_build.argtypes
    one = ((C.c_char_p * 1)(b"abc"), (C.c_size_t * 1)(3))
    others = (L.nxs_test_sugg_build(b"abd", 3, False, 1, 1, one[0], one[1], (C.c_uint * 1)(1), (C.c_uint64 * 1)(4)),
              L.nxs_test_compl_build(b"ab", 2, 1, 1, one[0], one[1], (C.c_uint64 * 1)(4)),
              L.nxs_test_wild_build(b"a*c", 3, 1, 1, one[0], one[1], (C.c_uint64 * 1)(4)),
              L.nxs_test_docterms_build(7, 1, 1, one[0], one[1], (C.c_uint * 1)(2), (C.c_uint64 * 1)(4), (C.c_float * 1)(1.5)))
    for sg in others:
        assert sg and L.nxs_sugg_count(sg) == 1
        docs = C.c_uint64(12345)
        assert not L.nxs_sugg_docs(sg, C.byref(docs)) and docs.value == 12345
        text = str(N._take(L.nxs_sugg_tojson(sg, None)))
        assert '"docs"' not in text and '"query"' not in text and '"count"' not in text
        L.nxs_sugg_release(sg)


def fbits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def triples(rng, n):
    """(c, df, term): c <= df; c = df, values above 2^24, equal shares from different pairs (2/4, 3/6), shares that
    differ as doubles and are equal as f32, equal c with different terms"""
    out = [(2, 4, 9), (3, 6, 5), (1, 2, 70), (5, 5, 1), (1, 1, 2), (7, 7, 4294967295), (1, 4294967295, 3),
           (4294967295, 4294967295, 6), ((1 << 24) + 1, (1 << 24) + 3, 11), ((1 << 24) + 1, (1 << 25) + 2, 12),
           (16777217, 33554434, 13), (16777216, 33554432, 14), (33554431, 33554432, 15), (33554430, 33554431, 16),
           (4, 8, 8), (4, 9, 10), (4, 7, 17)]
    seen = {t for _, _, t in out}
    while len(out) < n:
        df = rng.choice([rng.randint(1, 12), rng.randint(1, 1000), rng.randint(1 << 24, (1 << 32) - 1)])
        c = rng.choice([df, rng.randint(1, df), max(1, df // rng.randint(1, 9))])
        t = rng.randint(1, (1 << 32) - 1)
        if t not in seen:
            seen.add(t)
            out.append((c, df, t))
    return out


def test_the_key_orders_as_the_definition_does():
    L = N.lib()
    rng = random.Random(17)
    tr = triples(rng, 400)
    for c, df, t in tr:
        want = np.float32(np.float64(c) / np.float64(df))
        assert fbits(L.nxs_test_related_share(c, df)) == fbits(float(want)), (c, df)
    assert fbits(L.nxs_test_related_share(16777217, 33554434)) == fbits(L.nxs_test_related_share(16777216, 33554432))
    for order, rule in ((COUNT, lambda x: (-x[0], x[2])), (SHARE, lambda x: (-fbits(f32(x[0] / x[1])), x[2]))):
        keys = [L.nxs_test_related_key(order, c, df, t) for c, df, t in tr]
        assert len(set(keys)) == len(keys) and 0 not in keys and NONE not in keys
        assert [x for _, x in sorted(zip(keys, tr))] == sorted(tr, key=rule), order
        assert all(k & 0xffffffff == t for k, (_, _, t) in zip(keys, tr))
    # equal shares from different pairs: the term id decides
    k = L.nxs_test_related_key
    assert k(SHARE, 3, 6, 5) < k(SHARE, 2, 4, 9) < k(SHARE, 1, 2, 70) and k(SHARE, 4, 7, 17) < k(SHARE, 3, 6, 5)
    assert k(COUNT, 3, 6, 5) < k(COUNT, 2, 4, 9) and k(COUNT, 2, 2, 9) == k(COUNT, 2, 4, 9)


def test_the_predicate_and_the_host_ranker_against_numpy():
    L = N.lib()
    rng = random.Random(23)
    u32 = C.c_uint32
    ex = (u32 * 32)(*range(100, 132))
    assert L.nxs_test_related_eligible(3, 5, 3, 5, 7, ex, 32) and L.nxs_test_related_eligible(3, 5, 1, 1, 7, None, 0)
    assert not L.nxs_test_related_eligible(2, 5, 3, 5, 7, ex, 32) and not L.nxs_test_related_eligible(3, 4, 3, 5, 7, ex, 32)
    assert not L.nxs_test_related_eligible(3, 5, 3, 5, 100, ex, 32) and not L.nxs_test_related_eligible(3, 5, 3, 5, 131, ex, 32)
    assert L.nxs_test_related_eligible(3, 5, 3, 5, 131, ex, 31) and L.nxs_test_related_eligible(3, 5, 3, 5, 100, ex, 0)
    assert not L.nxs_test_related_eligible(0, 0, 1, 1, 7, None, 0)
    for trial in range(30):
        T = rng.choice([1, 2, 63, 64, 65, 300])
        big = trial % 3 == 0
        df = np.zeros(T + 1, dtype=np.uint32)
        c = np.zeros(T + 1, dtype=np.uint32)
        for t in range(1, T + 1):
            df[t] = rng.choice([0, rng.randint(1, 6), rng.randint(1, 40)]) if not big else rng.randint(1 << 24, (1 << 32) - 1)
            c[t] = rng.choice([0, int(df[t]), rng.randint(0, int(df[t]))]) if not big else \
                rng.choice([int(df[t]), rng.randint((1 << 24), int(df[t]))])
        excl = rng.sample(range(1, T + 1), min(T, rng.choice([0, 1, 3, 32])))
        for order in (COUNT, SHARE):
            for mincount, mindf, k in ((1, 1, 5), (2, 1, 1), (1, 3, 32), (3, 4, 7)):
                for n_excl in (0, len(excl)):
                    ok = [t for t in range(1, T + 1) if c[t] >= mincount and df[t] >= mindf and c[t] > 0
                          and t not in excl[:n_excl]]
                    if order == COUNT:
                        ok.sort(key=lambda t: (-int(c[t]), t))
                    else:
                        ok.sort(key=lambda t: (-fbits(float(np.float32(np.float64(c[t]) / np.float64(df[t])))), t))
                    out = (u32 * k)()
                    m = C.c_uint64(77)
                    got = L.nxs_test_related_rank(order, c.ctypes.data_as(C.POINTER(u32)), df.ctypes.data_as(C.POINTER(u32)),
                                                  T, mincount, mindf, (u32 * max(len(excl), 1))(*excl), n_excl, k, out,
                                                  C.byref(m))
                    ctx = (trial, T, order, mincount, mindf, k, n_excl)
                    assert got == min(k, len(ok)) and m.value == len(ok), ctx
                    assert list(out[:got]) == ok[:k], ctx
