"""Truth for the related-terms tests, computed in Python from the corpus a test wrote and the CPU oracle.

M = the doc ids of oracle.search(q, algo, limit=max(doc_count, 1), fuzzymatch) -- the doc set a total counts.  The
resolved token list is explain_truth.Truth.tokens.  c(t) = the docs of M that hold t and df(t) = the live docs
that hold t are counted from the docs the test wrote, removed docs left out.  s = numpy.float32(c / df), compared
by its bits.  Eligible terms are sorted by (-c, term id) under "count" and (-bits(s), term id) under "share"."""
import numpy as np

from explain_truth import Truth as ExTruth, bits, tf_of_docs


class Truth:
    """One snapshot: docs [(id, [token, ...])] as handed to nxsfmt, the removed ids, {term bytes: id}."""

    def __init__(self, oidx, docs, removed, term_ids):
        self.oidx = oidx
        self.ex = ExTruth(oidx, tf_of_docs(docs, removed))
        self.term_ids = dict(term_ids)
        self.df = {t: len(m) for t, m in self.ex.tf.items()}
        self.of_doc = {}
        for t, m in self.ex.tf.items():
            for d in m:
                self.of_doc.setdefault(d, []).append(t)
        self.memo = {}

    def doc_set(self, q, algo, fuzzymatch=False):
        """the doc ids of M (raises oracle_lib.SearchError for a query the oracle rejects)"""
        key = (q, algo, fuzzymatch)
        if key not in self.memo:
            try:
                self.memo[key] = [d for d, _ in self.oidx.search(q, algo=algo, limit=max(self.oidx.doc_count, 1),
                                                                  fuzzymatch=fuzzymatch)]
            except Exception as e:
                self.memo[key] = e
        if isinstance(self.memo[key], Exception):
            raise self.memo[key]
        return self.memo[key]

    def related(self, q, algo, k=5, order="count", mindf=1, mincount=1, include_self=False, fuzzymatch=False,
                rewritten=None, tokens=None):
        """-> ([(term bytes, c, df, s)] the first k, matches, n).  rewritten / tokens: the query the oracle runs and
        the resolved token list, where they are not the string's own (prefix and wildcard leaves)"""
        key = (q, algo, order, mindf, mincount, include_self, fuzzymatch, rewritten, None if tokens is None else tuple(tokens))
        if key not in self.memo:
            self.memo[key] = self.rows(q, algo, order, mindf, mincount, include_self, fuzzymatch, rewritten, tokens)
        rows, n = self.memo[key]
        return rows[:k], len(rows), n

    def rows(self, q, algo, order, mindf, mincount, include_self, fuzzymatch, rewritten, tokens):
        """-> (every eligible row in the order, n)"""
        M = self.doc_set(rewritten or q, algo, fuzzymatch)
        own = set() if include_self else set(self.ex.tokens(q, fuzzymatch) if tokens is None else tokens)
        c = {}
        for d in M:
            for t in self.of_doc.get(d, ()):
                c[t] = c.get(t, 0) + 1
        rows = [(t, n, self.df[t], float(np.float32(n / self.df[t]))) for t, n in c.items()
                if n >= mincount and self.df[t] >= mindf and t not in own]
        if order == "count":
            rows.sort(key=lambda r: (-r[1], self.term_ids[r[0]]))
        else:
            rows.sort(key=lambda r: (-bits(r[3]), self.term_ids[r[0]]))
        return rows, len(M)


def check_related(got, want, ctx):
    """an Index.related entry against Truth.related: everything, the floats by their bits"""
    rows, matches, n = want
    assert not isinstance(got, Exception), (ctx, got)
    assert [(t, c, df) for t, c, df, _ in got] == [(t, c, df) for t, c, df, _ in rows], (ctx, list(got), rows)
    assert [bits(s) for _, _, _, s in got] == [bits(s) for _, _, _, s in rows], (ctx, list(got), rows)
    assert got.matches == matches, (ctx, got.matches, matches)
    assert got.docs == n, (ctx, got.docs, n)
