"""CPU tier for prefix matching (nxs_index_complete, `term*` leaves): the C-ABI surface, the host ranker
against the Python truth, which leaves the prepare step reads as prefixes, the filter stages a prefix
takes, the parameters, the JSON writer, and the spliced program against the rewritten query's -- no GPU."""
import ctypes as C
import json
import random

import pytest

import nxsearch_amd as N
import oracle_lib as O
from complete_truth import Truth, big_corpus, big_prefixes, random_words, rewrite

NXS_H = ["nxs_index_complete", "nxs_index_complete_batch"]
NXS_GPU_H = ["nxsgpu_complete", "nxsgpu_complete_profile"]
HOOKS = ["nxs_test_complete_host", "nxs_test_complete_params", "nxs_test_compl_build", "nxs_test_prefix_query",
         "nxs_test_filter_prefix"]


def test_library_exports_the_complete_entry_points():
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
    assert callable(N.Index.complete) and callable(N.Index.complete_profile)


def host_rank(terms, dfs, prefix, k):
    """nxs_test_complete_host -> ([(id, df)], matches)"""
    L = N.lib()
    n = len(terms)
    L.nxs_test_complete_host.restype = None
    L.nxs_test_complete_host.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                         C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    arr = host_rank.cache.get(id(terms))
    if arr is None:
        arr = ((C.c_char_p * n)(*terms), (C.c_uint32 * n)(*[len(t) for t in terms]), (C.c_uint32 * n)(*dfs))
        host_rank.cache[id(terms)] = arr
    ids, df = (C.c_uint32 * k)(), (C.c_uint32 * k)()
    cnt, m = C.c_uint32(), C.c_uint32()
    L.nxs_test_complete_host(arr[0], arr[1], arr[2], n, prefix, len(prefix), k, ids, df, C.byref(cnt), C.byref(m))
    return [(ids[i], df[i]) for i in range(cnt.value)], m.value


host_rank.cache = {}


def test_host_ranker_against_the_truth():
    """The 2000-term vocabulary of the GPU tier (60 dead terms, blocks of equal df) and its 306 prefixes, every
    k; then the chunk-boundary and 0xFF vocabularies."""
    term_dfs, dead, words = big_corpus()
    terms = [w for w, _ in term_dfs] + list(dead)
    dfs = [df for _, df in term_dfs] + [0] * len(dead)
    truth = Truth(terms, dfs)
    nonempty = 0
    for k in (1, 5, 32):
        for p in big_prefixes(words):
            want = truth.rank(p, k)
            assert host_rank(terms, dfs, p, k) == want, (p, k)
            nonempty += bool(want[0])
    assert nonempty > 800
    assert all(tid != 1951 for tid, _ in truth.rank(words[1950], 32)[0])      # a dead word is not its own completion
    # a whole word is its own completion; equal df: the lower term id first
    m = truth.rank(b"a", 32)
    assert m[1] > 200 and m[0] == sorted(m[0], key=lambda r: (-r[1], r[0]))
    base = bytes(random.Random(5).choice(b"abcdef") for _ in range(200))
    terms2 = [base[:n] + s for n in (7, 8, 9, 15, 16, 17) for s in (b"x", b"y")] + [base[:66] + b"pqrs", base]
    terms2 += [b"a\xff", b"a\xffz", b"b"]
    dfs2 = [1 + i % 4 for i in range(len(terms2))]
    t2 = Truth(terms2, dfs2)
    for t in terms2:
        for n in range(1, len(t) + 1):
            assert host_rank(terms2, dfs2, t[:n], 32) == t2.rank(t[:n], 32), (t, n)
    assert t2.rank(b"a\xff", 5) == ([(16, 4), (15, 3)], 2) and t2.rank(b"a\xffz", 5) == ([(16, 4)], 1)


@pytest.fixture()
def nxs(tmp_path):
    h = N.Nxs(str(tmp_path))
    yield h
    h.close()


def complete_params(nxs, bools=None, **kv):
    """-> (complete_limit, prefixmatch, prefix_limit) as the calls read the parameters, or the NxsError"""
    L = N.lib()
    L.nxs_test_complete_params.restype = C.c_int
    L.nxs_test_complete_params.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint), C.POINTER(C.c_int),
                                           C.POINTER(C.c_uint)]
    p = None
    if kv or bools:
        p = L.nxs_params_create()
        for key, v in kv.items():
            L.nxs_params_set_uint(p, key.encode(), v)
        for key, v in (bools or {}).items():
            L.nxs_params_set_bool(p, key.encode(), v)
    k, pm, pl = C.c_uint(), C.c_int(), C.c_uint()
    try:
        if L.nxs_test_complete_params(nxs._h, p, C.byref(k), C.byref(pm), C.byref(pl)) != 0:
            return N.NxsError(*nxs.error())
        return k.value, bool(pm.value), pl.value
    finally:
        if p:
            L.nxs_params_release(p)


def test_parameters(nxs):
    assert complete_params(nxs) == (5, False, 8)
    assert complete_params(nxs, limit=3, suggest_limit=9) == (5, False, 8)        # other calls' keys
    assert complete_params(nxs, complete_limit=1) == (1, False, 8)
    assert complete_params(nxs, complete_limit=32, prefix_limit=32) == (32, False, 32)
    assert complete_params(nxs, bools={"prefixmatch": True}, prefix_limit=1) == (5, True, 1)
    assert complete_params(nxs, bools={"prefixmatch": False}) == (5, False, 8)
    for key, bad in (("complete_limit", 0), ("complete_limit", 33), ("prefix_limit", 0), ("prefix_limit", 33)):
        e = complete_params(nxs, **{key: bad})
        assert isinstance(e, N.NxsError) and e.code == 3 and key in e.msg, (key, bad, e)
    # the binding's keywords set the same keys; without them there are no params at all
    L = N.lib()
    u, b = C.c_uint64(), C.c_bool()
    assert N._make_params() is None and N._make_params(limit=None, total=False) is None
    p = N._make_params(prefixmatch=True, prefix_limit=4)
    assert L.nxs_params_get_uint(p, b"prefix_limit", C.byref(u)) == 0 and u.value == 4
    assert L.nxs_params_get_bool(p, b"prefixmatch", C.byref(b)) == 0 and b.value is True
    assert L.nxs_params_get_uint(p, b"limit", C.byref(u)) != 0
    L.nxs_params_release(p)


def build(prefix, rows, matches):
    """nxs_test_compl_build: a completion object by hand; rows = [(term, df)]"""
    L = N.lib()
    L.nxs_test_compl_build.restype = C.c_void_p
    L.nxs_test_compl_build.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint, C.POINTER(C.c_char_p),
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    n = len(rows)
    sg = L.nxs_test_compl_build(prefix, len(prefix), matches, n, (C.c_char_p * max(n, 1))(*[r[0] for r in rows]),
                                (C.c_size_t * max(n, 1))(*[len(r[0]) for r in rows]),
                                (C.c_uint64 * max(n, 1))(*[r[1] for r in rows]))
    assert sg
    return sg


def test_json_of_a_hand_built_completion():
    L = N.lib()
    nasty = b'q"u\\o\x01t\xc3\xa9'
    rows = [(nasty, 12), (b'q"plain', 1 << 40)]
    sg = build(b'q"', rows, 7)
    assert L.nxs_sugg_count(sg) == 2 and L.nxs_sugg_matches(sg) == 7 and not L.nxs_sugg_dropped(sg)
    term, ln, d, df = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64()
    assert L.nxs_sugg_get(sg, 1, C.byref(term), C.byref(ln), C.byref(d), C.byref(df))
    assert (C.string_at(term.value), ln.value, d.value, df.value) == (b'q"plain', 7, 5, 1 << 40)
    assert not L.nxs_sugg_get(sg, 2, C.byref(term), C.byref(ln), C.byref(d), C.byref(df))
    n = C.c_size_t()
    ptr = L.nxs_sugg_tojson(sg, C.byref(n))
    raw = C.string_at(ptr, n.value)
    N._libc.free(ptr)
    want = (b'{"prefix":"q\\"","completions":[{"term":"q\\"u\\\\o\\u0001t\xc3\xa9","df":12},'
            b'{"term":"q\\"plain","df":1099511627776}],"matches":7}')
    assert raw == want
    doc = json.loads(raw.decode("utf-8"))
    assert list(doc) == ["prefix", "completions", "matches"]
    assert [list(s) for s in doc["completions"]] == [["term", "df"]] * 2
    got = N._drain_sugg(sg)
    assert got == [(nasty, len(nasty) - 2, 12), (b'q"plain', 5, 1 << 40)] and got.matches == 7 and got.dropped is False
    assert N._drain_sugg(build(b"zz", [], 0), json=True) == '{"prefix":"zz","completions":[],"matches":0}'


def prefix_query(query, words, dfs, prefixmatch=True, limit=8, lowercase=True):
    """nxs_test_prefix_query -> (repr of the spliced query, leaves read as prefixes, their normalised bytes)"""
    L = N.lib()
    L.nxs_test_prefix_query.restype = C.c_void_p
    L.nxs_test_prefix_query.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.c_uint32, C.c_bool,
                                        C.c_bool, C.c_uint32, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
    n = len(words)
    npx = C.c_uint32()
    buf = C.create_string_buffer(4096)
    r = L.nxs_test_prefix_query(query.encode(), (C.c_char_p * max(n, 1))(*words), (C.c_uint32 * max(n, 1))(*dfs), n,
                                lowercase, prefixmatch, limit, C.byref(npx), buf, len(buf))
    return (N._take(r) if r else None), npx.value, buf.value.split(b"\n")[:-1]


WORDS = [b"ab", b"abc", b"abd", b"abe", b"b", b"cd", b"cde", b"e", b"micro*", b"*", b"abz"]
DFS = [3, 5, 5, 1, 2, 4, 9, 1, 1, 1, 0]


def test_which_leaves_are_prefixes():
    q = 'ab* AND "cd*" OR \'ab*\' OR * OR (CD* AND NOT e) ab*'
    assert prefix_query(q, WORDS, DFS)[1:] == (3, [b"ab", b"cd", b"ab"])
    # the flag off (or absent): no leaf is a prefix, the program is the parsed query's
    r, n, px = prefix_query(q, WORDS, DFS, prefixmatch=False)
    assert (n, px) == (0, []) and r == O.query_repr(q.replace("CD*", "cd*"))[0]
    assert prefix_query("*", WORDS, DFS)[1] == 0 and prefix_query("**", WORDS, DFS)[1:] == (1, [b"*"])
    assert prefix_query('"ab*"', WORDS, DFS)[1] == 0 and prefix_query("ab*c", WORDS, DFS)[1] == 0
    # operators and brackets next to the star
    assert prefix_query("(ab*)", WORDS, DFS)[1:] == (1, [b"ab"])
    assert prefix_query("AB* & cd* | e", WORDS, DFS)[1:] == (2, [b"ab", b"cd"])
    assert prefix_query("AB*", WORDS, DFS, lowercase=False)[1:] == (1, [b"AB"])


def test_spliced_program_is_the_rewritten_querys():
    truth = Truth(WORDS, DFS)
    assert truth.expansions(b"ab", 8) == [b"abc", b"abd", b"ab", b"abe"]          # df, then id; the dead term is out
    for limit in (1, 2, 8, 32):
        for q in ("ab*", "ab* AND e", "e AND NOT ab*", "(ab* OR cd*) AND e", "abc OR ab*", "ab* cd* b", "b (ab*) e",
                  "AB* AND NOT (cd* OR e)"):
            r = rewrite(q, truth, limit)
            assert "*" not in r and r != q
            got = prefix_query(q, WORDS, DFS, limit=limit)[0]
            assert got == O.query_repr(r.lower())[0] and got is not None, (q, limit, r)
    # no expansion: the leaf stays, as the empty set (its string is the leaf's own)
    assert prefix_query("zz* AND e", WORDS, DFS)[0] == O.query_repr("zz* AND e")[0]
    assert prefix_query("ab*", WORDS, DFS, limit=1)[0] == "`abc`"


def filter_prefix(basedir, stages, s):
    L = N.lib()
    L.nxs_test_filter_prefix.restype = C.c_void_p
    L.nxs_test_filter_prefix.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_int)]
    act = C.c_int()
    r = L.nxs_test_filter_prefix(str(basedir).encode(), stages, s, C.byref(act))
    return (N._take(r) if r else None), act.value


def filter_word(basedir, stages, s):
    L = N.lib()
    L.nxs_test_filter.restype = C.c_void_p
    L.nxs_test_filter.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_int)]
    act = C.c_int()
    r = L.nxs_test_filter(str(basedir).encode(), stages, s, C.byref(act))
    return (N._take(r) if r else None), act.value


def test_a_prefix_takes_the_normalizer_only(tmp_path):
    sw = tmp_path / "filters" / "stopwords"
    sw.mkdir(parents=True)
    (sw / "en").write_text("the\nth\n")
    # as a word: dropped / stemmed; as a prefix: kept, lowercased, not stemmed
    assert filter_word(tmp_path, 3, b"th") == (None, 0) and filter_word(tmp_path, 3, b"Running") == ("run", 1)
    assert filter_prefix(tmp_path, 3, b"th") == ("th", 1) and filter_prefix(tmp_path, 3, b"THE") == ("the", 1)
    assert filter_prefix(tmp_path, 3, b"Running") == ("running", 1)
    assert filter_prefix(tmp_path, 0, b"AZ\xc3\x9aL") == filter_word(tmp_path, 0, b"AZ\xc3\x9aL") == ("azul", 1)
