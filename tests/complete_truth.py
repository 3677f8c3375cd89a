"""Truth for the prefix-matching tests, computed in Python from the corpus a test wrote: the eligible terms of
a prefix p are the dictionary terms with df > 0 (df = the number of non-removed docs that hold the term) for
which term.startswith(p), in the order df descending, term id ascending.  For searches the truth is the
rewritten query: every `p*` leaf replaced by the parenthesised OR of its expansions."""
import random
import re


class Truth:
    """terms: list[bytes] in term-id order (id = index + 1); dfs: list[int]."""

    def __init__(self, terms, dfs):
        assert len(terms) == len(dfs)
        self.terms, self.dfs = list(terms), list(dfs)
        self.memo = {}

    def eligible(self, p):
        """[(-df, term id)] of every eligible term, in the order; each prefix once"""
        if p not in self.memo:
            self.memo[p] = sorted((-self.dfs[i], i + 1) for i, t in enumerate(self.terms)
                                  if self.dfs[i] > 0 and t.startswith(p))
        return self.memo[p]

    def rank(self, p, k=5):
        """-> ([(term id, df)] best k, matches)"""
        el = self.eligible(p)
        return [(tid, -ndf) for ndf, tid in el[:k]], len(el)

    def rank_terms(self, p, k=5):
        """the same as Index.complete returns it: (term bytes, distance = len(term) - len(p), df)"""
        rows, m = self.rank(p, k)
        return [(self.terms[tid - 1], len(self.terms[tid - 1]) - len(p), df) for tid, df in rows], m

    def expansions(self, p, limit=8):
        return [self.terms[tid - 1] for tid, _ in self.rank(p, limit)[0]]


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


def docs_of(term_dfs, dead=()):
    """doc j (id 10 (j + 1)) holds the terms with df > j; the dead terms live in doc 5 alone -- to be removed"""
    docs = [(5, list(dead))] if dead else []
    for j in range(max(df for _, df in term_dfs)):
        docs.append((10 * (j + 1), [t for t, df in term_dfs if df > j]))
    return docs, ([5] if dead else [])


def random_words(rng, n, alphabet="abcdef", lo=1, hi=10):
    """n distinct strings over the alphabet, lengths lo..hi"""
    seen, out = set(), []
    while len(out) < n:
        w = "".join(rng.choice(alphabet) for _ in range(rng.randint(lo, hi))).encode()
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def big_corpus():
    """The 2000-term a-f vocabulary of the suggestion tests (same generator, same seed): lengths 1-10; df 1..24
    with blocks of equal df; 60 terms dead (their only doc removed)."""
    rng = random.Random(20260)
    words = random_words(rng, 2000)
    dead = words[1940:]
    term_dfs = []
    for i, w in enumerate(words[:1940]):
        term_dfs.append((w, 7 if 400 <= i < 700 else 2 if 900 <= i < 1000 else rng.choice([1, 1, 2, 3, 5, 8, 13, 24])))
    return term_dfs, dead, words


def big_prefixes(words):
    """300 prefixes of 1-6 bytes taken from the words, plus the edge ones"""
    rng = random.Random(20261)
    px = []
    for _ in range(300):
        w = rng.choice(words)
        px.append(w[:rng.randint(1, min(6, len(w)))])
    px += [b"a", b"f", words[3], words[1950], px[0], b"abcdefabcdefabcdef"]
    return px


# a free-form leaf that ends in a star: not inside quotes, at least one byte in front of the star
_LEAF = re.compile(r"""(?<![^\s(])([^\s()"'*]+)\*(?=[\s)]|$)""")

NO_MATCH = "qqqqqqqqqqqqqqqq"       # in no test dictionary and beyond the fuzzy tolerance of all their terms


def rewrite(query, truth, limit=8, lowercase=True):
    """Q -> R: every `p*` leaf becomes (e1 OR e2 OR ... OR em); no expansion: a leaf that resolves to nothing"""
    def sub(m):
        p = m.group(1).lower() if lowercase else m.group(1)
        ex = truth.expansions(p.encode(), limit)
        if not ex:
            return NO_MATCH
        return "(" + " OR ".join(e.decode() for e in ex) + ")"
    return _LEAF.sub(sub, query)
