"""Validates the oracle restatement against the GENUINE reference
src/algo/{levdist,bktree,deque,heap}.c.  The reference's answers for the seeded
inputs below are recorded in tests/golden/reference_algo.json.gz (written by
tests/golden/make_reference_algo.py from oracle/_ref/libnxsref.so, which
oracle/Makefile compiles in place from a reference checkout), so these tests
need nothing outside the repository.  Where oracle/_ref has been built, every
case is also checked against the live reference library."""
import gzip
import json
import os
import random

import pytest

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_algo.json.gz")

BKTREE_SETS = [(1, 300, "abcd"), (2, 3000, "abcdefghijklmnopqrstuvwxyz"), (3, 2000, "ab")]


def rand_word(rng, lo=1, hi=12, alphabet="abcdefgh"):
    return "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))).encode()


# ---- the seeded inputs (shared with tests/golden/make_reference_algo.py) ----

def levdist_pairs():
    rng = random.Random(11)
    pairs = []
    for _ in range(20000):
        a = rand_word(rng, 0, 24, "abcxyz\xc4\x85 ")
        b = rand_word(rng, 0, 24, "abcxyz\xc4\x85 ")
        pairs.append((a, b))
    # long strings (row > 255, uint16 row)
    for _ in range(20):
        a = rand_word(rng, 200, 700, "ab")
        b = rand_word(rng, 200, 700, "ab")
        pairs.append((a, b))
    return pairs


def bktree_set(seed, n, alphabet):
    """(words, [(query, tol), ...])"""
    rng = random.Random(seed)
    words = []
    while len(words) < n:
        w = rand_word(rng, 1, 10, alphabet)
        if rng.random() < 0.05 and words:
            w = rng.choice(words)          # duplicates are rejected (EEXIST)
        words.append(w)
    searches = []
    for _ in range(300):
        q = bytearray(rng.choice(words))
        if q and rng.random() < 0.8:
            q[rng.randrange(len(q))] = ord(rng.choice(alphabet))
        if rng.random() < 0.3:
            q += rng.choice(alphabet).encode()
        for tol in (0, 1, 2, 3):
            searches.append((bytes(q), tol))
    return words, searches


def long_words_set():
    """(words, queries): distances above 63 share one bucket (bktree.c:196)"""
    rng = random.Random(5)
    words = [rand_word(rng, 1, 4, "ab") for _ in range(50)]
    words += [rand_word(rng, 70, 120, "abc") for _ in range(30)]
    rng.shuffle(words)
    return words, [rand_word(rng, 1, 5, "ab") for _ in range(50)]


def topk_trials():
    rng = random.Random(7)
    trials = []
    for _ in range(400):
        n = rng.randint(0, 300)
        k = rng.choice([1, 2, 3, 5, 10, 17, 64, 1000])
        levels = rng.choice([1, 2, 3, 8, 1000])
        ids = list(range(n, 0, -1))                      # descending doc id
        sc = [float(rng.randrange(levels)) / 4 + 0.25 for _ in ids]
        trials.append((ids, sc, k))
    return trials


# ---- the reference's answers: recorded, and live where oracle/_ref is built ----

_golden = None


def golden_ref():
    global _golden
    if _golden is None:
        with gzip.open(GOLDEN, "rt") as f:
            _golden = json.load(f)
    return _golden


def bk_answers(tree, searches):
    return [list(tree.search(q, tol)) for q, tol in searches]


def topk_answer(ids, sc, k):
    return [list(e) for e in O.ref_topk(ids, sc, k)]


def test_levdist_matches_reference_on_random_strings():
    pairs = levdist_pairs()
    want = golden_ref()["levdist"]
    assert len(want) == len(pairs)
    R = O.ref()
    for (a, b), w in zip(pairs, want):
        assert O.levdist(a, b) == w, (a, b)
        if R is not None:
            assert R.ref_levdist(a, len(a), b, len(b)) == w, (a, b)


@pytest.mark.parametrize("seed,n,alphabet", BKTREE_SETS)
def test_bktree_search_order_matches_reference(seed, n, alphabet):
    words, searches = bktree_set(seed, n, alphabet)
    want = golden_ref()["bktree"][str(seed)]
    assert len(want) == len(searches)
    orc = O.BKTree(words)
    got = bk_answers(orc, searches)
    orc.close()
    if O.ref() is not None:
        ref = O.RefBKTree(words)
        assert bk_answers(ref, searches) == want
        ref.close()
    for (q, tol), (r1, n1), (r2, n2) in zip(searches, want, got):
        assert r1 == r2, (q, tol)
        assert n1 == n2


def test_bktree_long_words_clamped_slot():
    words, queries = long_words_set()
    searches = [(q, 2) for q in queries]
    want = golden_ref()["bktree_long_words"]
    orc = O.BKTree(words)
    got = bk_answers(orc, searches)
    orc.close()
    if O.ref() is not None:
        ref = O.RefBKTree(words)
        assert bk_answers(ref, searches) == want
        ref.close()
    assert got == want


def test_topk_matches_reference_heap_with_massive_ties():
    trials = topk_trials()
    want = golden_ref()["topk"]
    assert len(want) == len(trials)
    live = O.ref() is not None
    for trial, ((ids, sc, k), w) in enumerate(zip(trials, want)):
        if live:
            assert topk_answer(ids, sc, k) == w, (trial, len(ids), k)
        assert [list(e) for e in O.topk(ids, sc, k)] == w, (trial, len(ids), k)
