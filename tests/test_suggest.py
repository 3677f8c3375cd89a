"""GPU tier (`-m gpu`) for spelling suggestions: Index.suggest -> nxs_index_suggest_batch -> nxsgpu_suggest.

Truth is computed here, in Python (suggest_truth.Truth), from the corpus the test itself wrote: df = the
number of non-removed docs that hold the term, distance = the oracle's levdist, order = distance
ascending, df descending, term id ascending.  Every token of every test is compared in full: terms (ids),
distances, dfs, order, the list's length and `matches`."""
import ctypes as C
import json
import random

import pytest

import nxsearch_amd as N
import nxsfmt
from suggest_truth import Truth, misspell, random_words

pytestmark = pytest.mark.gpu

KS = (1, 5, 32)
MAXDISTS = (1, 2)


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def truth_of_docs(docs, removed, term_ids):
    terms = [None] * len(term_ids)
    for t, i in term_ids.items():
        terms[i - 1] = t
    dfs = [0] * len(terms)
    for did, toks in docs:
        if did in removed:
            continue
        for t in set(x.encode() if isinstance(x, str) else x for x in toks):
            dfs[term_ids[t] - 1] += 1
    return Truth(terms, dfs)


def docs_of(term_dfs, dead=()):
    """doc j (id 10 (j + 1)) holds the terms with df > j; the dead terms live in doc 5 alone -- to be removed"""
    docs = [(5, list(dead))] if dead else []
    for j in range(max(df for _, df in term_dfs)):
        docs.append((10 * (j + 1), [t for t, df in term_dfs if df > j]))
    return docs, ([5] if dead else [])


def make_index(nxs, tmp_path, name, term_dfs, dead=(), lowercase=False):
    docs, removed = docs_of(term_dfs, dead)
    t, d, term_ids = nxsfmt.write_index(str(tmp_path), name, docs, removed=removed)
    truth = truth_of_docs(docs, removed, term_ids)
    for term, df in term_dfs:
        assert truth.dfs[term_ids[term] - 1] == df
    for term in dead:
        assert truth.dfs[term_ids[term] - 1] == 0
    return nxs.open_files(t, d, lowercase=lowercase), truth


def check(gidx, truth, tokens, k=None, maxdist=None, ctx=None):
    """Index.suggest against the truth, every token in full -> the lists"""
    got = gidx.suggest(tokens, limit=k, maxdist=maxdist)
    assert len(got) == len(tokens)
    for tok, g in zip(tokens, got):
        want, m = truth.rank_terms(tok, 5 if k is None else k, 2 if maxdist is None else maxdist)
        assert not isinstance(g, N.NxsError), (ctx, tok, g)
        assert list(g) == want, (ctx, tok, k, maxdist)
        assert g.matches == m and g.dropped is False, (ctx, tok, k, maxdist, g.matches, m)
    return got


def shim(gidx, tokens, k, maxdist):
    """nxsgpu_suggest itself -> [([(term id, distance, df)], matches)]"""
    L = N.lib()
    n = len(tokens)
    offs = [0]
    for t in tokens:
        offs.append(offs[-1] + len(t))
    ids, dist, df = (C.c_uint32 * (n * k))(), (C.c_uint8 * (n * k))(), (C.c_uint32 * (n * k))()
    cnt, m = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    r = L.nxsgpu_suggest(gidx.device, b"".join(tokens) + b"\0" * 16, (C.c_uint32 * (n + 1))(*offs), n, maxdist, k,
                         ids, dist, df, cnt, m)
    assert r == 0, L.nxsgpu_last_error()
    return [([(ids[i * k + j], dist[i * k + j], df[i * k + j]) for j in range(cnt[i])], m[i]) for i in range(n)]


def set_route(monkeypatch, gidx, route):
    """NXS_GPU_SUGGEST: None = the device pass, "host" = the host ranker for everything"""
    if route is None:
        monkeypatch.delenv("NXS_GPU_SUGGEST", raising=False)
    else:
        monkeypatch.setenv("NXS_GPU_SUGGEST", route)
    gidx.reconfigure()


# ---- the shared 2000-term vocabulary -------------------------------------------------------

def big_corpus():
    """2000 terms over a-f, lengths 1-10; df 1..24 with blocks of equal df; 60 of them dead (their only doc
    removed); 300 misspelt tokens."""
    rng = random.Random(20260)
    words = random_words(rng, 2000)
    dead = words[1940:]
    term_dfs = []
    for i, w in enumerate(words[:1940]):
        term_dfs.append((w, 7 if 400 <= i < 700 else 2 if 900 <= i < 1000 else rng.choice([1, 1, 2, 3, 5, 8, 13, 24])))
    tokens = [misspell(rng, rng.choice(words)) for _ in range(290)]
    tokens += [b"a", b"f", b"ab", b"fe", b"cab", words[3], words[1950], tokens[0], tokens[0], b"abcdefabcdefabcdef"]
    assert len(tokens) == 300
    return term_dfs, dead, tokens, words


@pytest.fixture(scope="module")
def big(nxs, tmp_path_factory):
    term_dfs, dead, tokens, words = big_corpus()
    gidx, truth = make_index(nxs, tmp_path_factory.mktemp("big"), "big", term_dfs, dead=dead)
    yield gidx, truth, tokens, words
    gidx.close()


# ---- 1. random parity ----------------------------------------------------------------------

@pytest.mark.parametrize("route", [None, "host"], ids=["device", "host"])
def test_random_parity(big, monkeypatch, route):
    """300 tokens (k_fz_filter runs two grid.y slices) and a batch of one, every k and maxdist, on the
    device pass and on the host ranker; the shim's term ids against the truth's."""
    gidx, truth, tokens, _ = big
    set_route(monkeypatch, gidx, route)
    gidx.suggest_profile(reset=True)
    try:
        for k in KS:
            for maxdist in MAXDISTS:
                check(gidx, truth, tokens, k, maxdist, route)
                check(gidx, truth, tokens[5:6], k, maxdist, route)
        assert check(gidx, truth, tokens[:7]) == check(gidx, truth, tokens[:7], 5, 2)      # the defaults
        for (rows, m), tok in zip(shim(gidx, tokens, 5, 2), tokens):
            assert (rows, m) == truth.rank(tok, 5, 2), tok
        host = gidx.suggest_profile()["host_tokens"]
        assert host == (0 if route is None else 6 * 301 + 14 + 300)
    finally:
        set_route(monkeypatch, gidx, None)


# ---- 2. candidate-count edges --------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_candidate_count_edges(nxs, tmp_path, n):
    """Exactly 0 (every doc removed), 1, 255, 256 and 257 eligible candidates: one lane, a full workgroup
    of k_fz_filter less one, exactly one, one more."""
    rng = random.Random(100 + n)
    words = random_words(rng, max(n, 6), lo=2, hi=6)
    if n == 0:
        docs = [(5, words[:3]), (6, words[3:])]
        t, d, term_ids = nxsfmt.write_index(str(tmp_path), "edge", docs, removed=[5, 6])
        gidx, truth = nxs.open_files(t, d), truth_of_docs(docs, {5, 6}, term_ids)
    else:
        gidx, truth = make_index(nxs, tmp_path, "edge", [(w, rng.randint(1, 3)) for w in words[:n]])
    assert sum(1 for x in truth.dfs if x > 0) == n
    tokens = [misspell(rng, rng.choice(words)) for _ in range(40)] + [words[0], b"ab", b"a"]
    for k in (1, 32):
        got = check(gidx, truth, tokens, k, 2, n)
        if n == 0:
            assert all(g == [] and g.matches == 0 for g in got)
    if n:
        assert check(gidx, truth, [words[0]], 1, 1, n)[0][0][:2] == (words[0], 0)      # the exact hit comes first
    gidx.close()


# ---- 3. length window ----------------------------------------------------------------------

@pytest.mark.parametrize("L", [3, 8])
def test_length_window(nxs, tmp_path, L):
    """Tokens of length L - 3 .. L + 3 made from one term of length L by deletions and insertions: two
    edits match, three never do."""
    S = b"abcdefgh"[:L]
    gidx, truth = make_index(nxs, tmp_path, "win%d" % L, [(S, 2), (b"qrstuvwxyzqrstu", 1), (b"mnmnmnmnmnmn", 3)])
    tokens = [S[:L - 3], S[:L - 2], S[:L - 1], S, S + b"x", S + b"xy", S + b"xyz",
              S[3:], S[2:], S[1:], b"x" + S, b"yx" + S, b"zyx" + S, S[:1] + b"x" + S[1:] + b"y"]
    for maxdist in MAXDISTS:
        got = check(gidx, truth, tokens, 5, maxdist, L)
        for tok, g in zip(tokens, got):
            d = abs(len(tok) - L)
            assert (g == [(S, d, 2)] and g.matches == 1) if d <= maxdist else (g == [] and g.matches == 0), (tok, maxdist)
    gidx.close()


def test_short_tokens_against_many_short_terms(nxs, tmp_path):
    """Tokens of 1 and 2 bytes are within 2 of nearly every term of up to 3 bytes: segments far larger
    than k -- the list is the exact top k, `matches` the exact count."""
    rng = random.Random(33)
    words = random_words(rng, 236, lo=1, hi=3)
    gidx, truth = make_index(nxs, tmp_path, "short", [(w, rng.choice([1, 2, 2, 3, 9])) for w in words])
    tokens = [bytes([a]) for a in b"abcdef"] + [bytes([a, b]) for a in b"abcdef" for b in b"abcdef"] + [b"g", b"gh", b""]
    for k in KS:
        got = check(gidx, truth, tokens, k, 2, k)
        assert min(g.matches for g in got[:42]) > 64 and all(len(g) == k for g in got[:42])
    check(gidx, truth, tokens, 32, 1)
    gidx.close()


# ---- 4. ties -------------------------------------------------------------------------------

@pytest.mark.parametrize("distinct", [False, True], ids=["equal-df", "distinct-df"])
def test_ties(nxs, tmp_path, distinct):
    """40 terms at distance 1 of one token: with equal df the first k by term id, with distinct df by df
    descending; a distance-2 term with a huge df never precedes them."""
    tok = b"abcdef"
    near = [tok[:p] + bytes([c]) + tok[p + 1:] for p in range(6) for c in b"ghijklm"][:40]
    rng = random.Random(8)
    order = list(range(40))
    rng.shuffle(order)
    term_dfs = [(b"abcdxy", 60)] + [(w, 1 + order[i] if distinct else 3) for i, w in enumerate(near)]
    gidx, truth = make_index(nxs, tmp_path, "ties", term_dfs)
    for k in KS:
        g = check(gidx, truth, [tok], k, 2, k)[0]
        assert g.matches == 41 and all(d == 1 for _, d, _ in g)
        if distinct:
            assert [df for _, _, df in g] == list(range(40, 40 - k, -1))
        else:
            # term ids are first-seen order: "abcdxy" is 1, near[i] is i + 2
            assert [t for t, _, _ in g] == near[:k]
    g = check(gidx, truth, [tok], 32, 1)[0]
    assert g.matches == 40
    g = gidx.suggest([tok], limit=32, maxdist=2)[0]
    assert len(g) == 32 and (b"abcdxy", 2, 60) not in g
    gidx.close()


# ---- 5. signature collisions ---------------------------------------------------------------

def test_signature_collisions(nxs, tmp_path):
    """The screen hashes bytes by & 31: 'a', 'A' and '!' are one bit.  Terms that differ from the token only
    by such bytes pass the screen whatever their number; the exact distance drops those beyond 2."""
    tok = b"abcde"
    terms = [b"abcde", b"Abcde", b"AbcdE", b"ABCde", b"!BCDe", b"aBCDE", b"!\"#$%", b"ABCDE"]
    gidx, truth = make_index(nxs, tmp_path, "sig", [(w, i + 1) for i, w in enumerate(terms)])
    gidx.set_profiling(True)
    gidx.suggest_profile(reset=True)
    g = check(gidx, truth, [tok], 32, 2)[0]
    prof = gidx.suggest_profile(reset=True)
    gidx.set_profiling(False)
    assert g == [(b"abcde", 0, 1), (b"Abcde", 1, 2), (b"AbcdE", 2, 3)] and g.matches == 3
    # all eight went through the screen, three were matches
    assert prof["passes"] == 1 and prof["survivors"] == 8 and prof["matches"] == 3 and prof["ms"] > 0
    check(gidx, truth, [tok, b"ABCDE", b"!bcde"], 5, 1)
    gidx.close()


# ---- 6. the bit-vector boundary ------------------------------------------------------------

def test_myers_boundary(nxs, tmp_path):
    """Tokens of 63 .. 66 bytes against terms of 64 .. 68 bytes: up to 64 the device's bit-vector distance,
    beyond it the host ranker, silently -- which also finds the 67-byte term for the 65-byte token."""
    rng = random.Random(6)
    B = bytes(rng.choice(b"abcdef") for _ in range(68))
    other = bytes(rng.choice(b"abcdef") for _ in range(66))
    X = B[:30] + b"x" + B[31:]
    terms = [B[:64], B[:65], B[:66], B[:67], B[:68], X[:64], X[:66], X[:67], other]
    gidx, truth = make_index(nxs, tmp_path, "myers", [(w, 1 + i % 3) for i, w in enumerate(terms)])
    tokens = [B[:63], B[:64], B[:65], B[:66], X[:63], X[:65], other[:64], other + b"ab"]
    gidx.suggest_profile(reset=True)
    for maxdist in MAXDISTS:
        got = check(gidx, truth, tokens, 32, maxdist)
    assert gidx.suggest_profile()["host_tokens"] == 2 * 4           # B[:65], B[:66], X[:65], other + "ab"
    assert (B[:67], 2, 1 + 3 % 3) in got[2] and got[2][0] == (B[:65], 0, 2)
    assert (B[:66], 2, 3) in got[1]                                 # the longest term a 64-byte token reaches
    check(gidx, truth, tokens, 1, 2)
    gidx.close()


# ---- 7. the subtree the BK walk never enters -----------------------------------------------

def test_slot_63_subtree(nxs, tmp_path):
    """Root "x", then a 65-byte term T (distance to the root >= 63: the clamped slot, which bktree_search
    never enters) and two terms within 1 of T below it.  The fuzzy search finds nothing for a token next to
    them; the suggestions list all three."""
    rng = random.Random(63)
    T = bytes(rng.choice(b"abcdef") for _ in range(65))
    T1 = T[:64] + (b"a" if T[64:] != b"a" else b"b")
    T2 = T[:64]
    docs = [(10, [b"x", T, T1, T2]), (20, [T, T2]), (30, [T2])]
    t, d, term_ids = nxsfmt.write_index(str(tmp_path), "slot63", docs)
    assert [term_ids[w] for w in (b"x", T, T1, T2)] == [1, 2, 3, 4]
    gidx, truth = nxs.open_files(t, d), truth_of_docs(docs, (), term_ids)
    tok = (T[:10] + (b"c" if T[10:11] != b"c" else b"d") + T[11:])[:64]
    g = check(gidx, truth, [tok], 5, 2)[0]
    assert g == [(T2, 1, 3), (T, 2, 2), (T1, 2, 1)] and g.matches == 3
    assert gidx.fuzzy([tok]) == [0]
    assert check(gidx, truth, [tok], 5, 1)[0] == [(T2, 1, 3)]
    gidx.close()


# ---- 8. snapshots --------------------------------------------------------------------------

def truth_of_events(ev):
    term_ids, docs, removed = {}, [], set()
    for e in ev:
        if e[0] == "add":
            docs.append((e[1], e[2]))
            for w in e[2]:
                term_ids.setdefault(w.encode(), len(term_ids) + 1)
        else:
            removed.add(e[1])
    return truth_of_docs(docs, removed, term_ids)


def test_suggestions_follow_a_refresh(nxs, tmp_path):
    ev = [("add", 10, ["apple", "maple", "zebra"]), ("add", 20, ["apple", "apply"]), ("add", 30, ["ample", "apple"]),
          ("add", 40, ["apply", "zebra"]), ("add", 50, ["ample"])]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 262144)
    open(d, "wb").write(dimg + b"\0" * 262144)
    gidx = nxs.open_files(t, d)

    def publish():
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        nxsfmt.publish_in_place(t, d, timg, dimg)
        return truth_of_events(ev)
    tokens = [b"appla", b"zebra", b"amplo"]
    old_truth = truth_of_events(ev)
    before = check(gidx, old_truth, tokens, 5, 2, "snapshot 0")
    assert before[0] == [(b"apple", 1, 3), (b"apply", 1, 2), (b"ample", 2, 2)] and before[0].matches == 3
    ev += [("rm", 20), ("rm", 40)]                           # every doc of "apply"
    after = check(gidx, publish(), tokens, 5, 2, "removal")
    assert after[0] == [(b"apple", 1, 2), (b"ample", 2, 2)] and after[0].matches == before[0].matches - 1
    ev.append(("add", 60, ["applq", "zebra"]))               # a new term next to the token
    newer = check(gidx, publish(), tokens, 5, 2, "append")
    assert newer[0] == [(b"apple", 1, 2), (b"applq", 1, 1), (b"ample", 2, 2)] and newer[0].matches == 3
    # what was answered before a publish belongs to its snapshot
    assert before[0] == old_truth.rank_terms(b"appla", 5, 2)[0] and (b"apply", 1, 2) in before[0]
    gidx.close()


# ---- 9. overflow ---------------------------------------------------------------------------

def test_overflowing_queues_change_nothing(big, monkeypatch):
    """NXS_GPU_FUZZY_CAND at its minimum: 300 short tokens against 2000 terms leave far more survivors than
    the queues hold -- the passes are repeated with fewer tokens, down to single tokens with queues
    grown to the screen's bound; the answers are those of the unconstrained run and of the truth."""
    gidx, truth, _, words = big
    rng = random.Random(9)
    tokens = [misspell(rng, rng.choice(words)[:4]) for _ in range(290)] + [b"a", b"b", b"ab", b"ba", b"abc"] * 2
    plain = {k: check(gidx, truth, tokens, k, 2, "plain") for k in (5, 32)}
    gidx.suggest_profile(reset=True)
    assert gidx.suggest_profile()["overflow_reruns"] == 0
    monkeypatch.setenv("NXS_GPU_FUZZY_CAND", "1024")
    gidx.reconfigure()
    try:
        for k in (5, 32):
            got = check(gidx, truth, tokens, k, 2, "constrained")
            assert got == plain[k] and [g.matches for g in got] == [g.matches for g in plain[k]]
        assert gidx.suggest_profile()["overflow_reruns"] > 0
    finally:
        monkeypatch.delenv("NXS_GPU_FUZZY_CAND")
        gidx.reconfigure()


# ---- 10. beside batches in flight ----------------------------------------------------------

def test_beside_batches_in_flight(big):
    """A batch whose misspelt terms are still with the device's fuzzy pass, then suggest, then the batch's
    end: both as if called alone.  The same with two batches in flight."""
    gidx, truth, tokens, words = big
    rng = random.Random(10)
    toks = [t.decode() for t in tokens[:120] if len(t) >= 3]
    qa = ["%s OR %s" % (rng.choice(toks), rng.choice(toks)) for _ in range(96)]
    qb = ["%s AND %s" % (rng.choice(toks), words[rng.randrange(1900)].decode()) for _ in range(80)]
    alone_a, alone_b = gidx.search_batch(qa, limit=10), gidx.search_batch(qb, limit=10)
    sugg_alone = check(gidx, truth, tokens, 5, 2, "alone")
    gidx.search_batch_begin(qa, limit=10)
    assert check(gidx, truth, tokens, 5, 2, "one in flight") == sugg_alone
    assert gidx.search_batch_end() == alone_a
    gidx.search_batch_begin(qa, limit=10)
    gidx.search_batch_begin(qb, limit=10)
    assert check(gidx, truth, tokens[:40], 32, 1, "two in flight") == check(gidx, truth, tokens[:40], 32, 1)
    assert gidx.search_batch_end() == alone_a
    assert check(gidx, truth, tokens, 5, 2, "one left") == sugg_alone
    assert gidx.search_batch_end() == alone_b


# ---- 11. consistency with fuzzymatch -------------------------------------------------------

def test_the_fuzzy_winner_is_a_suggestion(big):
    """For misspelt tokens whose whole match set fits the list (k = 32): the term the fuzzy search resolves
    the token to, if it has df > 0, is in the list."""
    gidx, truth, _, words = big
    rng = random.Random(11)
    longish = [w for w in words if len(w) >= 7]
    tokens = [misspell(rng, rng.choice(longish), edits=rng.randint(1, 2)) for _ in range(100)]
    got = check(gidx, truth, tokens, 32, 2)
    checked = 0
    for tok, g, tid in zip(tokens, got, gidx.fuzzy(tokens)):
        if g.matches <= 32 and tid and truth.dfs[tid - 1] > 0:
            assert truth.terms[tid - 1] in [t for t, _, _ in g], (tok, tid)
            checked += 1
    assert checked >= 50


# ---- 12. API surface -----------------------------------------------------------------------

def suggest_one(gidx, token, limit=None, maxdist=None, as_json=False):
    """nxs_index_suggest()"""
    L = N.lib()
    p = N._suggest_params(limit, maxdist)
    tb = N._b(token)
    try:
        sg = L.nxs_index_suggest(gidx._h, p, tb, len(tb))
    finally:
        if p:
            L.nxs_params_release(p)
    if not sg:
        gidx.nxs._raise()
    return N._drain_sugg(sg, as_json)


def test_filters_lowercase(nxs, tmp_path):
    gidx, truth = make_index(nxs, tmp_path, "lc", [(b"hello", 2), (b"hallo", 3), (b"help", 1), (b"world", 1)], lowercase=True)
    want = check(gidx, truth, [b"hello"], 5, 2)[0]
    assert want == [(b"hello", 0, 2), (b"hallo", 1, 3), (b"help", 2, 1)]
    got = gidx.suggest(["HELLO", "hello", "HeLLo", "hello"])
    assert got == [want] * 4 and all(g.matches == 3 for g in got)          # duplicates: equal lists
    # one call = a batch of one; the length is the caller's
    assert suggest_one(gidx, "HELLO") == want
    sg = N.lib().nxs_index_suggest(gidx._h, None, b"HELLOxyz", 5)
    assert sg and N._drain_sugg(sg) == want
    one = suggest_one(gidx, "HELL", limit=2, maxdist=1)
    assert (list(one), one.matches) == truth.rank_terms(b"hell", 2, 1)
    # the JSON round-trips to the same tuples, the token is the filtered one
    doc = json.loads(suggest_one(gidx, "HELLO", as_json=True))
    assert list(doc) == ["token", "suggestions", "matches"] and doc["token"] == "hello" and doc["matches"] == 3
    assert [(s["term"].encode(), s["distance"], s["df"]) for s in doc["suggestions"]] == want
    assert gidx.suggest(["HELLO"], json=True) == [suggest_one(gidx, "hello", as_json=True)]
    # parameters out of range fail the call and name the key
    for kw, key in ((dict(limit=0), "suggest_limit"), (dict(limit=33), "suggest_limit"),
                    (dict(maxdist=0), "suggest_maxdist"), (dict(maxdist=3), "suggest_maxdist")):
        with pytest.raises(N.NxsError) as e:
            gidx.suggest(["hello"], **kw)
        assert e.value.code == 3 and key in e.value.msg
    # an accessor past the end
    L = N.lib()
    sg = L.nxs_index_suggest(gidx._h, None, b"hello", 5)
    assert sg and L.nxs_sugg_count(sg) == 3
    term, ln, dd, df = C.c_void_p(), C.c_size_t(), C.c_uint(), C.c_uint64()
    assert L.nxs_sugg_get(sg, 2, C.byref(term), C.byref(ln), C.byref(dd), C.byref(df))
    assert (C.string_at(term.value), ln.value, dd.value, df.value) == (b"help", 4, 2, 1)
    assert not L.nxs_sugg_get(sg, 3, C.byref(term), C.byref(ln), C.byref(dd), C.byref(df))
    L.nxs_sugg_release(sg)
    assert gidx.suggest([]) == []
    gidx.close()


def test_default_filters_drop_stop_words(tmp_path):
    base = tmp_path / "b"
    docs = [(1, ["azul", "henry"]), (2, ["azur", "azul"]), (3, ["the"])]
    t, d, term_ids = nxsfmt.write_index(str(base), "sw", docs, filters=["normalizer", "stopwords"])
    sw = base / "filters" / "stopwords"
    sw.mkdir(parents=True)
    (sw / "en").write_text("the\nof\n")
    truth = truth_of_docs(docs, (), term_ids)
    with N.Nxs(str(base)) as n2:
        idx = n2.open_index("sw")
        got = idx.suggest(["the", "AZÚL", "THE", "azul", "henri"])
        assert got[0] == [] and got[0].matches == 0 and got[0].dropped is True and got[2].dropped is True
        for g, plain in zip(got[1:2] + got[3:], (b"azul", b"azul", b"henri")):
            assert (list(g), g.matches, g.dropped) == truth.rank_terms(plain, 5, 2) + (False,)
        assert got[1] == [(b"azul", 0, 2), (b"azur", 1, 1)]
        assert json.loads(idx.suggest(["the"], json=True)[0]) == {"token": "", "suggestions": [], "matches": 0}
        idx.close()


def test_shards_and_communicators(nxs, tmp_path):
    docs, _ = docs_of([(b"hello", 2), (b"hallo", 3), (b"help", 1)])
    t, d, term_ids = nxsfmt.write_index(str(tmp_path), "sh", docs)
    truth = truth_of_docs(docs, (), term_ids)
    sh = nxs.open_shard(t, d, 0, 1)
    with pytest.raises(N.NxsError) as e:
        sh.suggest(["hello"])
    assert e.value.code == 3 and e.value.msg == "suggest is not available on a doc shard"
    sh.close()
    gidx = nxs.open_files(t, d)
    gidx.shard(0, 1, nxs.shard_unique_id())
    check(gidx, truth, [b"hello", b"helo"], 5, 2, "world 1")
    gidx.search_batch_begin(["hello OR helo"], limit=5)
    check(gidx, truth, [b"hello", b"helo"], 5, 2, "world 1, a batch in flight")
    assert len(gidx.search_batch_end()) == 1
    gidx.shard(0, 1, None)
    check(gidx, truth, [b"hello"], 5, 2, "detached")
    gidx.close()
