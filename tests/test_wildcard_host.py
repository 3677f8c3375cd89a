"""CPU tier for wildcard matching (nxs_index_wildcard, `*` / `?` leaves): the C-ABI surface, the matcher
(nxs_wild.h) against a regex, the host ranker against the Python truth, the parameters, which leaves the
prepare step reads as patterns and how it normalises them, the spliced program against the rewritten query's,
and the JSON writer -- no GPU."""
import ctypes as C
import json

import pytest

import nxsearch_amd as N
import oracle_lib as O
from wild_truth import (WildTruth, big_patterns, big_truth, generator_strength, literals, normalise, pattern_regex,
                        rewrite)

NXS_H = ["nxs_index_wildcard", "nxs_index_wildcard_batch"]
NXS_GPU_H = ["nxsgpu_wildcard", "nxsgpu_wildcard_profile"]
HOOKS = ["nxs_test_wild_match", "nxs_test_wild_match_inl", "nxs_test_wild_host", "nxs_test_wild_params",
         "nxs_test_wild_normalize", "nxs_test_wild_build", "nxs_test_wild_query"]


def test_library_exports_the_wildcard_entry_points():
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
    assert callable(N.Index.wildcard) and callable(N.Index.wildcard_profile)


def test_the_generator_is_strong_enough():
    """300 patterns: >= 250 non-empty, >= 100 with more than 32 matches, >= 30 with more than 256, >= 100 that
    begin with a metacharacter -- from the truth alone"""
    truth, words = big_truth()
    ne, m32, m256, lead = generator_strength(truth, big_patterns(words))
    assert ne >= 250 and m32 >= 100 and m256 >= 30 and lead >= 100, (ne, m32, m256, lead)


def matchers():
    L = N.lib()
    for f in (L.nxs_test_wild_match, L.nxs_test_wild_match_inl):
        f.restype = C.c_int
        f.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    # host form, and the device's: the first 8 bytes from the node's inline copy
    return (lambda t, p: bool(L.nxs_test_wild_match(t, len(t), p, len(p))),
            lambda t, p: bool(L.nxs_test_wild_match_inl(t, len(t), p, len(p))))


def test_matcher_against_the_regex_on_the_vocabulary():
    truth, words = big_truth()
    for match in matchers():
        for p in big_patterns(words):
            rx = pattern_regex(p)
            for w in words:
                assert match(w, p) == bool(rx.fullmatch(w)), (w, p)


def test_matcher_hand_cases():
    for match in matchers():
        def same(t, p):
            got = match(t, p)
            assert got == bool(pattern_regex(p).fullmatch(t)), (t, p, got)
            return got
        # the empty term
        assert same(b"", b"*") and same(b"", b"**") and not same(b"", b"?") and not same(b"", b"a") and same(b"", b"")
        assert not same(b"a", b"")
        # `?` is exactly one byte
        assert same(b"x", b"?") and not same(b"xy", b"?") and same(b"xy", b"??") and not same(b"x", b"??")
        # a star may be empty, at either end
        assert same(b"a", b"a*") and same(b"a", b"*a") and same(b"a", b"*a*") and not same(b"b", b"*a*")
        assert same(b"ab", b"a*") and not same(b"ba", b"a*") and same(b"ba", b"*a") and same(b"bab", b"*a*")
        # a product, not an exponent
        run = b"a" * 200
        assert same(run + b"b", b"*a*a*a*b") and not same(run, b"*a*a*a*b")
        # (120 stars: a backtracking regex would not come back, so no regex here)
        assert not match(run, b"*a" * 120 + b"*b") and match(run + b"b", b"*a" * 120 + b"*b")
        # a 255-byte pattern
        p255 = b"ab?" * 84 + b"ab*"
        assert len(p255) == 255
        assert same(b"abc" * 84 + b"ab", p255) and same(b"abc" * 84 + b"abzz", p255) and not same(b"abc" * 84 + b"a", p255)
        # a 300-byte term, the pattern's metacharacter at the inline boundary (7 / 8 / 9)
        t300 = bytes(97 + (i * 7 + i // 5) % 6 for i in range(300))
        for n in (7, 8, 9):
            assert same(t300, t300[:n] + b"*") and same(t300, t300[:n] + b"?" + t300[n + 1:])
            assert same(t300, t300[:n] + b"*" + t300[-n:]) and same(t300, b"*" + t300[n:])
            assert not same(t300, t300[:n] + b"?" + t300[n + 2:]) and same(t300, b"?" * n + t300[n:])
            wrong = bytearray(t300)
            wrong[n] ^= 1
            assert not same(bytes(wrong), t300) and same(bytes(wrong), t300[:n] + b"?" + t300[n + 1:])
            assert same(t300[:n], t300[:n]) and same(t300[:n], b"?" * n) and not same(t300[:n], b"?" * (n + 1))
        # 65535 bytes, the most a str_len carries
        big = bytes(97 + i % 5 for i in range(65535))
        assert same(big, b"*" + big[-9:]) and same(big, big[:9] + b"*" + big[-9:]) and not same(big, b"*f*")
        # bytes 0x80-0xFF are bytes
        hi = bytes(range(0x80, 0x100))
        assert same(hi, hi) and same(hi, b"\x80*\xff") and same(hi, b"?" * 128) and not same(hi, b"\x80*\xfe")
        assert same(b"\xc3\xa9", b"??") and not same(b"\xc3\xa9", b"?") and same(b"a\xffz", b"a\xff*")
        # `**` is `*`
        for t in (b"", b"a", b"abc", b"ba"):
            for p, q in ((b"**", b"*"), (b"a**", b"a*"), (b"**a", b"*a"), (b"a**c", b"a*c")):
                assert same(t, p) == same(t, q)


def host_rank(terms, dfs, pat, k):
    """nxs_test_wild_host -> ([(id, df)], matches)"""
    L = N.lib()
    n = len(terms)
    L.nxs_test_wild_host.restype = None
    L.nxs_test_wild_host.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                     C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    arr = host_rank.cache.get(id(terms))
    if arr is None:
        arr = ((C.c_char_p * n)(*terms), (C.c_uint32 * n)(*[len(t) for t in terms]), (C.c_uint32 * n)(*dfs))
        host_rank.cache[id(terms)] = arr
    ids, df = (C.c_uint32 * k)(), (C.c_uint32 * k)()
    cnt, m = C.c_uint32(), C.c_uint32()
    L.nxs_test_wild_host(arr[0], arr[1], arr[2], n, pat, len(pat), k, ids, df, C.byref(cnt), C.byref(m))
    return [(ids[i], df[i]) for i in range(cnt.value)], m.value


host_rank.cache = {}


def test_host_ranker_against_the_truth():
    truth, words = big_truth()
    terms, dfs = truth.terms, truth.dfs
    for k in (1, 5, 32):
        for p in big_patterns(words):
            assert host_rank(terms, dfs, p, k) == truth.rank(p, k), (p, k)
    # equal-df blocks come out in term-id order (terms 400..699 all have df 7)
    rows, m = host_rank(terms, dfs, b"*a*", 32)
    assert m > 256 and rows == sorted(rows, key=lambda r: (-r[1], r[0]))
    block = [tid for tid, df in truth.rank(b"*a*", m)[0] if df == 7]
    assert len(block) > 32 and block == sorted(block)
    # dead terms are never returned and never counted
    dead = words[1950]
    assert dfs[1950] == 0 and pattern_regex(b"*" + dead[1:]).fullmatch(dead)
    rows, m = host_rank(terms, dfs, b"*" + dead[1:], 32)
    assert 1951 not in [tid for tid, _ in rows] and m == len(truth.eligible(b"*" + dead[1:]))
    assert host_rank(terms, dfs, dead[:-1] + b"?", 32)[1] == sum(
        1 for i, t in enumerate(terms) if dfs[i] and len(t) == len(dead) and t[:-1] == dead[:-1])


@pytest.fixture()
def nxs(tmp_path):
    h = N.Nxs(str(tmp_path))
    yield h
    h.close()


def wild_params(nxs, bools=None, **kv):
    """-> (wildcard_limit, wildcardmatch, wildcard_terms) as the calls read the parameters, or the NxsError"""
    L = N.lib()
    L.nxs_test_wild_params.restype = C.c_int
    L.nxs_test_wild_params.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_int),
                                       C.POINTER(C.c_uint)]
    p = None
    if kv or bools:
        p = L.nxs_params_create()
        for key, v in kv.items():
            L.nxs_params_set_uint(p, key.encode(), v)
        for key, v in (bools or {}).items():
            L.nxs_params_set_bool(p, key.encode(), v)
    k, wm, wt = C.c_uint(), C.c_int(), C.c_uint()
    try:
        if L.nxs_test_wild_params(nxs._h, p, C.byref(k), C.byref(wm), C.byref(wt)) != 0:
            return N.NxsError(*nxs.error())
        return k.value, bool(wm.value), wt.value
    finally:
        if p:
            L.nxs_params_release(p)


def test_parameters(nxs):
    assert wild_params(nxs) == (5, False, 8)
    assert wild_params(nxs, limit=3, complete_limit=9, prefix_limit=3) == (5, False, 8)     # other calls' keys
    assert wild_params(nxs, wildcard_limit=1) == (1, False, 8)
    assert wild_params(nxs, wildcard_limit=32, wildcard_terms=32) == (32, False, 32)
    assert wild_params(nxs, bools={"wildcardmatch": True}, wildcard_terms=1) == (5, True, 1)
    assert wild_params(nxs, bools={"wildcardmatch": False}) == (5, False, 8)
    assert wild_params(nxs, bools={"prefixmatch": True}) == (5, False, 8)
    for key, bad in (("wildcard_limit", 0), ("wildcard_limit", 33), ("wildcard_terms", 0), ("wildcard_terms", 33)):
        e = wild_params(nxs, **{key: bad})
        assert isinstance(e, N.NxsError) and e.code == 3 and key in e.msg, (key, bad, e)
    L = N.lib()
    u, b = C.c_uint64(), C.c_bool()
    assert N._make_params() is None
    p = N._make_params(wildcardmatch=True, wildcard_terms=4)
    assert L.nxs_params_get_uint(p, b"wildcard_terms", C.byref(u)) == 0 and u.value == 4
    assert L.nxs_params_get_bool(p, b"wildcardmatch", C.byref(b)) == 0 and b.value is True
    assert L.nxs_params_get_bool(p, b"prefixmatch", C.byref(b)) != 0
    L.nxs_params_release(p)


def wild_query(query, words, dfs, prefixmatch=False, wildcardmatch=True, prefix_limit=8, terms=8, lowercase=True):
    """nxs_test_wild_query -> (repr of the spliced query, [b"p <prefix>" | b"w <pattern>"] in source order, errcode)"""
    L = N.lib()
    L.nxs_test_wild_query.restype = C.c_void_p
    L.nxs_test_wild_query.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_bool,
                                      C.c_bool, C.c_bool, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p,
                                      C.c_size_t, C.POINTER(C.c_int)]
    n = len(words)
    nl, err = C.c_uint32(), C.c_int()
    buf = C.create_string_buffer(8192)
    r = L.nxs_test_wild_query(query.encode() if isinstance(query, str) else query, (C.c_char_p * max(n, 1))(*words),
                              (C.c_uint32 * max(n, 1))(*dfs), n, lowercase, prefixmatch, wildcardmatch, prefix_limit,
                              terms, C.byref(nl), buf, len(buf), C.byref(err))
    leaves = buf.value.split(b"\n")[:-1]
    assert len(leaves) == nl.value
    return (N._take(r) if r else None), leaves, err.value


WORDS = [b"ab", b"abc", b"abd", b"abe", b"b", b"cd", b"cde", b"e", b"micro*", b"*", b"abz", b"microsoft", b"micron",
         b"misoft", b"mi*soft", b"acd"]
DFS = [3, 5, 5, 1, 2, 4, 9, 1, 1, 1, 0, 6, 2, 3, 1, 2]


def test_which_leaves_are_patterns():
    q = 'a?c AND "c?*" OR \'*d\' OR * OR (C*E AND NOT e) ?? *b? ab'
    r, leaves, err = wild_query(q, WORDS, DFS)
    assert leaves == [b"w a?c", b"w c*e", b"w *b?"] and err == 0 and r is not None
    # the flag off (or absent): no leaf is a pattern, the program is the parsed query's
    r, leaves, _ = wild_query(q, WORDS, DFS, wildcardmatch=False)
    assert leaves == [] and r == O.query_repr(q.replace("C*E", "c*e"))[0]
    # quoted leaves, a lone star, `??` and other leaves without a literal byte stay ordinary
    for plain in ('"mi*soft"', "'a?c'", "*", "?", "??", "**", "*?*", "abc"):
        assert wild_query(plain, WORDS, DFS)[1] == [], plain
        assert wild_query(plain, WORDS, DFS, prefixmatch=True)[1] == [], plain
    # `micro*`: a prefix leaf under both flags, a wildcard leaf under wildcardmatch alone -- with identical
    # expansions when the two limits are equal
    both = wild_query("micro*", WORDS, DFS, prefixmatch=True, prefix_limit=3, terms=3)
    alone = wild_query("micro*", WORDS, DFS, prefixmatch=False, terms=3)
    assert both[1] == [b"p micro"] and alone[1] == [b"w micro*"]
    assert both[0] == alone[0] == O.query_repr("microsoft OR micron OR micro*")[0]
    assert wild_query("micro*", WORDS, DFS, prefixmatch=True, wildcardmatch=False)[1] == [b"p micro"]
    # under both flags anything else with a metacharacter is a wildcard leaf
    assert wild_query("mi*soft *soft mi?ro* micro** a*", WORDS, DFS, prefixmatch=True)[1] == \
        [b"w mi*soft", b"w *soft", b"w mi?ro*", b"w micro*", b"p a"]
    # operators and brackets next to the metacharacters
    assert wild_query("(a?c)", WORDS, DFS)[1] == [b"w a?c"]
    assert wild_query("A?C & *d | e", WORDS, DFS)[1] == [b"w a?c", b"w *d"]


def test_normalisation_is_per_piece():
    assert wild_query("MI*Soft", WORDS, DFS)[1] == [b"w mi*soft"]
    assert wild_query("MI*Soft", WORDS, DFS, lowercase=False)[1] == [b"w MI*Soft"]
    assert wild_query("A***B??C**", WORDS, DFS)[1] == [b"w a*b??c*"]
    assert normalise(b"A***B??C**", True) == b"a*b??c*"
    # an over-long pattern fails its query: NXS_ERR_INVALID; 255 bytes after the stars collapse is served
    r, leaves, err = wild_query("a" * 255 + "*", WORDS, DFS)
    assert r is None and err == 3
    r, leaves, err = wild_query("a" * 254 + "****", WORDS, DFS)
    assert err == 0 and leaves == [b"w " + b"a" * 254 + b"*"]


def wild_normalize(pat, lowercase=True):
    """nxs_test_wild_normalize: the pattern through the explicit-length path of nxs_index_wildcard ->
    (result, normalised bytes, literal bytes)"""
    L = N.lib()
    L.nxs_test_wild_normalize.restype = C.c_int
    L.nxs_test_wild_normalize.argtypes = [C.c_bool, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    buf = C.create_string_buffer(1024)
    n, lit = C.c_size_t(), C.c_size_t()
    r = L.nxs_test_wild_normalize(lowercase, pat, len(pat), buf, len(buf), C.byref(n), C.byref(lit))
    return (r, buf.raw[:n.value], lit.value) if r == 1 else (r, None, None)


def test_a_pattern_with_an_embedded_nul():
    """The length is the caller's: a NUL inside a literal piece is a byte of that piece, before and behind a
    metacharacter, and the bytes behind it are normalised and counted like any others."""
    assert wild_normalize(b"AB\0CDEF*Z") == (1, b"ab\0cdef*z", 8)
    assert wild_normalize(b"AB\0CDEF*Z", lowercase=False) == (1, b"AB\0CDEF*Z", 8)
    long_p = b"AB\0" + b"CDEFG" * 7 + b"*z"                                 # 40 bytes, the NUL at 2
    assert len(long_p) == 40 and wild_normalize(long_p) == (1, long_p.lower(), 39)
    assert wild_normalize(b"\0*\0\0?X\0") == (1, b"\0*\0\0?x\0", 5)
    assert wild_normalize(b"\0") == (1, b"\0", 1) and wild_normalize(b"*\0**") == (1, b"*\0*", 1)
    assert wild_normalize(b"a" * 127 + b"\0" + b"B" * 127) == (1, b"a" * 127 + b"\0" + b"b" * 127, 255)
    assert wild_normalize(b"a" * 128 + b"\0" + b"B" * 127)[0] == -3         # 256 bytes: too long
    assert wild_normalize(b"*?*")[0] == 0
    # the matcher takes the NUL as a byte too
    match = matchers()[0]
    assert match(b"ab\0cdefxz", b"ab\0cdef*z") and not match(b"ab", b"ab\0cdef*z") and match(b"a\0b", b"a?b")


def test_spliced_program_is_the_rewritten_querys():
    truth = WildTruth(WORDS, DFS)
    assert truth.expansions(b"ab?", 8) == [b"abc", b"abd", b"abe"]           # df, then id; the dead term is out
    assert truth.expansions(b"mi*soft", 8) == [b"microsoft", b"misoft", b"mi*soft"]
    assert truth.expansions(b"*d", 8) == [b"abd", b"cd", b"acd"] and truth.expansions(b"a?d", 8) == [b"abd", b"acd"]
    for terms in (1, 2, 8, 32):
        for q in ("ab?", "ab? AND e", "e AND NOT *d", "(ab? OR c*) AND e", "abc OR a?c", "a?? *d b", "b (MI*soft) e",
                  "A* AND NOT (?d OR e)", "*b* ?"):
            r = rewrite(q, truth, terms)
            assert r != q, (q, r)
            got = wild_query(q, WORDS, DFS, terms=terms)[0]
            assert got == O.query_repr(r.lower())[0] and got is not None, (q, terms, r)
    # mixed with a prefix leaf, each kind with its own limit
    for q in ("ab* AND *d", "a?c OR micro*", "(mi*soft OR ab*) AND NOT c*e"):
        r = rewrite(q, truth, 2, prefixmatch=True, prefix_limit=3)
        got = wild_query(q, WORDS, DFS, prefixmatch=True, prefix_limit=3, terms=2)[0]
        assert got == O.query_repr(r)[0] and got is not None, (q, r)
    assert rewrite("ab* AND *d", truth, 2, prefixmatch=True, prefix_limit=3) == "(abc OR abd OR ab) AND (abd OR cd)"
    # no expansion: the leaf stays, as the empty set (its string is the leaf's own)
    assert wild_query("z?z AND e", WORDS, DFS)[0] == O.query_repr("z?z AND e")[0]
    assert wild_query("ab?", WORDS, DFS, terms=1)[0] == "`abc`"


def build(pattern, rows, matches):
    """nxs_test_wild_build: a wildcard object by hand; rows = [(term, df)]"""
    L = N.lib()
    L.nxs_test_wild_build.restype = C.c_void_p
    L.nxs_test_wild_build.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint, C.POINTER(C.c_char_p),
                                      C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    n = len(rows)
    sg = L.nxs_test_wild_build(pattern, len(pattern), matches, n, (C.c_char_p * max(n, 1))(*[r[0] for r in rows]),
                               (C.c_size_t * max(n, 1))(*[len(r[0]) for r in rows]),
                               (C.c_uint64 * max(n, 1))(*[r[1] for r in rows]))
    assert sg
    return sg


def test_json_of_a_hand_built_wildcard_object():
    L = N.lib()
    nasty = b'q"u\\o\x01t\xc3\xa9'
    rows = [(nasty, 12), (b'q"plain', 1 << 40)]
    sg = build(b'q"*?', rows, 7)
    assert L.nxs_sugg_count(sg) == 2 and L.nxs_sugg_matches(sg) == 7 and not L.nxs_sugg_dropped(sg)
    term, ln, d, df = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64()
    assert L.nxs_sugg_get(sg, 1, C.byref(term), C.byref(ln), C.byref(d), C.byref(df))
    assert (C.string_at(term.value), ln.value, d.value, df.value) == (b'q"plain', 7, 5, 1 << 40)
    assert not L.nxs_sugg_get(sg, 2, C.byref(term), C.byref(ln), C.byref(d), C.byref(df))
    n = C.c_size_t()
    ptr = L.nxs_sugg_tojson(sg, C.byref(n))
    raw = C.string_at(ptr, n.value)
    N._libc.free(ptr)
    want = (b'{"pattern":"q\\"*?","terms":[{"term":"q\\"u\\\\o\\u0001t\xc3\xa9","df":12},'
            b'{"term":"q\\"plain","df":1099511627776}],"matches":7}')
    assert raw == want
    doc = json.loads(raw.decode("utf-8"))
    assert list(doc) == ["pattern", "terms", "matches"]
    assert [list(s) for s in doc["terms"]] == [["term", "df"]] * 2
    got = N._drain_sugg(sg)
    assert got == [(nasty, len(nasty) - literals(b'q"*?'), 12), (b'q"plain', 5, 1 << 40)] and got.matches == 7
    assert got.dropped is False
    assert N._drain_sugg(build(b"z?z", [], 0), json=True) == '{"pattern":"z?z","terms":[],"matches":0}'
