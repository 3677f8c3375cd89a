"""Truth for the spelling-suggestion tests, computed in Python: the eligible terms of a token are the
dictionary terms with df > 0 within `maxdist` of it by the oracle's levdist (pinned to the genuine
levdist.c), in the order distance ascending, df descending, term id ascending."""
import random

import oracle_lib as O


class Truth:
    """terms: list[bytes] in term-id order (id = index + 1); dfs: list[int]."""

    def __init__(self, terms, dfs):
        assert len(terms) == len(dfs)
        self.terms, self.dfs = list(terms), list(dfs)
        self.by_len = {}
        for i, t in enumerate(self.terms):
            self.by_len.setdefault(len(t), []).append(i)
        self.memo = {}

    def near(self, token):
        """[(distance, term index)] of every term within 2, dead ones included; each token once.
        (Only lengths within 2 of the token's are tried: the distance is at least the length difference.)"""
        if token not in self.memo:
            out = []
            for ln in range(max(len(token) - 2, 0), len(token) + 3):
                for i in self.by_len.get(ln, ()):
                    d = O.levdist(self.terms[i], token)
                    if d <= 2:
                        out.append((d, i))
            self.memo[token] = out
        return self.memo[token]

    def rank(self, token, k=5, maxdist=2):
        """-> ([(term id, distance, df)] best k, matches)"""
        el = sorted((d, -self.dfs[i], i + 1) for d, i in self.near(token) if d <= maxdist and self.dfs[i] > 0)
        return [(tid, d, -ndf) for d, ndf, tid in el[:k]], len(el)

    def rank_terms(self, token, k=5, maxdist=2):
        """the same with the terms' bytes, as Index.suggest returns them"""
        rows, m = self.rank(token, k, maxdist)
        return [(self.terms[tid - 1], d, df) for tid, d, df in rows], m


def random_words(rng, n, alphabet="abcdef", lo=1, hi=10):
    """n distinct strings over the alphabet, lengths lo..hi (the short ones run out: whatever exists)"""
    seen, out = set(), []
    while len(out) < n:
        w = "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))).encode()
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def misspell(rng, w, alphabet="abcdef", edits=None):
    """w with 0..3 random edits"""
    w = bytearray(w)
    for _ in range(rng.randint(0, 3) if edits is None else edits):
        op = rng.randint(0, 2)
        if op == 0 and len(w) > 1:
            del w[rng.randrange(len(w))]
        elif op == 1:
            w.insert(rng.randint(0, len(w)), ord(rng.choice(alphabet)))
        elif w:
            w[rng.randrange(len(w))] = ord(rng.choice(alphabet))
    return bytes(w)
