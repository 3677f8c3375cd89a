"""Truth for the wildcard-matching tests, computed in Python from the corpus a test wrote: the eligible terms of a
pattern are the dictionary terms with df > 0 (df = the number of non-removed docs that hold the term) that the
pattern matches as a whole -- a regex built from it (re.escape on the literals, `*` -> `.*`, `?` -> `.`, re.S,
fullmatch on bytes; not fnmatch, which reads `[`) -- in the order df descending, term id ascending.  For
searches the truth is the rewritten query: every wildcard leaf replaced by the parenthesised OR of its
expansions (and, with prefixmatch, every `p*` leaf by its completions)."""
import random
import re

from complete_truth import NO_MATCH, Truth, big_corpus, truth_of_docs as _px_truth_of_docs


def pattern_regex(pat):
    out = b""
    for c in pat:
        b = bytes([c])
        out += b".*" if b == b"*" else b"." if b == b"?" else re.escape(b)
    return re.compile(out, re.S)


def literals(pat):
    return sum(1 for c in pat if c not in b"*?")


def normalise(pat, lowercase=False):
    """the literal pieces lowercased (ASCII, the `lowercase` index option), runs of stars collapsed"""
    if lowercase:
        pat = pat.lower()
    return re.sub(rb"\*+", b"*", pat)


class WildTruth:
    """terms: list[bytes] in term-id order (id = index + 1); dfs: list[int]."""

    def __init__(self, terms, dfs):
        assert len(terms) == len(dfs)
        self.terms, self.dfs = list(terms), list(dfs)
        self.memo = {}
        self.prefix = Truth(terms, dfs)

    def eligible(self, pat):
        """[(-df, term id)] of every eligible term, in the order; each pattern once"""
        if pat not in self.memo:
            rx = pattern_regex(pat)
            self.memo[pat] = sorted((-self.dfs[i], i + 1) for i, t in enumerate(self.terms)
                                    if self.dfs[i] > 0 and rx.fullmatch(t))
        return self.memo[pat]

    def rank(self, pat, k=5):
        """-> ([(term id, df)] best k, matches)"""
        el = self.eligible(pat)
        return [(tid, -ndf) for ndf, tid in el[:k]], len(el)

    def rank_terms(self, pat, k=5):
        """the same as Index.wildcard returns it: (term bytes, distance = len(term) - literal bytes, df)"""
        rows, m = self.rank(pat, k)
        lit = literals(pat)
        return [(self.terms[tid - 1], len(self.terms[tid - 1]) - lit, df) for tid, df in rows], m

    def expansions(self, pat, limit=8):
        return [self.terms[tid - 1] for tid, _ in self.rank(pat, limit)[0]]


def truth_of_docs(docs, removed, term_ids):
    t = _px_truth_of_docs(docs, removed, term_ids)
    return WildTruth(t.terms, t.dfs)


def big_patterns(words, n=300, seed=20262):
    """n patterns over the a-f vocabulary: `*tail`, `head*tail`, `*mid*`, `?` substitutions, `?` with a trailing
    star, `a*b*c` with and without a leading star"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        w = rng.choice(words)
        shape = len(out) % 7
        if shape == 0:                                          # *tail
            p = b"*" + w[-rng.randint(1, min(3, len(w))):]
        elif shape == 1:                                        # head*tail
            v = rng.choice(words)
            p = w[:rng.randint(1, min(2, len(w)))] + b"*" + v[-rng.randint(1, min(2, len(v))):]
        elif shape == 2:                                        # *mid*
            a = rng.randrange(len(w))
            p = b"*" + w[a:a + rng.randint(1, 2)] + b"*"
        elif shape == 3:                                        # ? substitutions
            if len(w) < 2:
                continue
            b = bytearray(w)
            for pos in rng.sample(range(len(w)), rng.randint(1, min(3, len(w) - 1))):
                b[pos] = ord("?")
            p = bytes(b)
        elif shape == 4:                                        # ? with a trailing star
            if len(w) < 3:
                continue
            b = bytearray(w[:rng.randint(2, min(4, len(w)))])
            b[rng.randrange(len(b))] = ord("?")
            if not literals(bytes(b)):
                continue
            p = bytes(b) + b"*"
        elif shape == 5:                                        # a*b*c
            p = b"*".join(bytes([rng.choice(b"abcdef")]) for _ in range(3))
        else:                                                   # *a*b*c
            p = b"*" + b"*".join(bytes([rng.choice(b"abcdef")]) for _ in range(rng.randint(2, 3)))
            if rng.random() < 0.5:
                p += b"*"
        out.append(p)
    return out


def generator_strength(truth, patterns):
    """-> (non-empty, > 32 matches, > 256 matches, begin with a metacharacter)"""
    ms = [len(truth.eligible(p)) for p in patterns]
    return (sum(1 for m in ms if m), sum(1 for m in ms if m > 32), sum(1 for m in ms if m > 256),
            sum(1 for p in patterns if p[:1] in (b"*", b"?")))


def big_truth():
    """the truth of complete_truth.big_corpus(): 1940 live terms and 60 dead ones, ids in vocabulary order"""
    term_dfs, dead, words = big_corpus()
    return WildTruth([w for w, _ in term_dfs] + list(dead), [df for _, df in term_dfs] + [0] * len(dead)), words


# a free-form leaf: not inside quotes
_LEAF = re.compile(r"""(?<![^\s(])([^\s()"']+)(?=[\s)]|$)""")


def rewrite(query, truth, limit=8, lowercase=True, prefixmatch=False, prefix_limit=8):
    """Q -> R: every wildcard leaf becomes (e1 OR e2 OR ... OR em); no expansion: a leaf that resolves to nothing.
    prefixmatch: a literal followed by one trailing star is a prefix leaf, with prefix_limit."""
    def sub(m):
        leaf = m.group(1)
        meta = sum(leaf.count(c) for c in "*?")
        if not meta or meta == len(leaf):
            return leaf
        pat = normalise(leaf.encode(), lowercase)
        if prefixmatch and meta == 1 and leaf.endswith("*"):
            ex = truth.prefix.expansions(pat[:-1], prefix_limit)
        else:
            ex = truth.expansions(pat, limit)
        if not ex:
            return NO_MATCH
        return "(" + " OR ".join(e.decode() for e in ex) + ")"
    return _LEAF.sub(sub, query)
