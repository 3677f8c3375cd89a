"""Truth for the similar-documents tests, computed in Python from the corpus a test wrote and the CPU oracle.

The term vector of a live doc d: w(t, d) is the oracle's one-token score (explain_truth.Truth.contrib: the docs a
term's negative rank leaves out are missing from that map, search.c:251-256, so such a term is not eligible), tf
comes from the docs, df is the number of live docs that hold the term.  The eligible terms are sorted by (-w, term
id), w compared through its f32 bits (w >= 0: the bits order as the floats do).  For `similar` the truth is the
rewritten query string (e1 OR e2 OR ... OR em) on the oracle, at limit + 1 with the source doc dropped here."""
from explain_truth import Truth as ExTruth, bits, tf_of_docs


class Truth:
    """One snapshot: docs [(id, [token, ...])] as handed to nxsfmt, the removed ids, {term bytes: id}."""

    def __init__(self, oidx, docs, removed, term_ids):
        self.oidx = oidx
        self.ex = ExTruth(oidx, tf_of_docs(docs, removed))
        self.term_ids = dict(term_ids)
        self.live = sorted(d for d, _ in docs if d not in set(removed))
        self.df = {t: len(m) for t, m in self.ex.tf.items()}
        self.of_doc = {}
        for t, m in self.ex.tf.items():
            for d in m:
                self.of_doc.setdefault(d, []).append(t)
        self.memo = {}

    def vector(self, doc, algo, mindf=1):
        """[(term bytes, tf, df, w)] of every eligible term of a live doc, in the order"""
        key = (doc, algo, mindf)
        if key not in self.memo:
            rows = []
            for t in self.of_doc.get(doc, []):
                m = self.ex.contrib(t, algo)
                if self.df[t] >= mindf and doc in m:
                    assert m[doc] >= 0.0
                    rows.append((-bits(m[doc] + 0.0), self.term_ids[t], t))
            rows.sort()
            self.memo[key] = [(t, self.ex.tf[t][doc], self.df[t], self.ex.contrib(t, algo)[doc]) for _, _, t in rows]
        return self.memo[key]

    def rank(self, doc, algo, k=5, mindf=1):
        """-> (the first k rows, matches)"""
        v = self.vector(doc, algo, mindf)
        return v[:k], len(v)

    def expansions(self, doc, algo, terms=8, mindf=2):
        return [t for t, _, _, _ in self.vector(doc, algo, mindf)[:terms]]

    def rewritten(self, doc, algo, terms=8, mindf=2):
        """the query a similar search of `doc` stands for, or None: no expansion"""
        ex = self.expansions(doc, algo, terms, mindf)
        return "(" + " OR ".join(e.decode() for e in ex) + ")" if ex else None

    def similar(self, doc, algo, limit=10, terms=8, mindf=2, include_self=False):
        """-> ([(doc id, score)], total, the rewritten query or None)"""
        q = self.rewritten(doc, algo, terms, mindf)
        if q is None:
            return [], 0, None
        total = len(self.oidx.search(q, algo=algo, limit=max(self.oidx.doc_count, 1), fuzzymatch=False))
        if include_self:
            return self.oidx.search(q, algo=algo, limit=limit, fuzzymatch=False), total, q
        res = [r for r in self.oidx.search(q, algo=algo, limit=limit + 1, fuzzymatch=False) if r[0] != doc]
        return res[:limit], total - 1, q


def check_vector(got, want, ctx):
    """an Index.doc_terms entry against Truth.rank: everything, the floats by their bits"""
    rows, matches = want
    assert not isinstance(got, Exception), (ctx, got)
    assert [(t, tf, df) for t, tf, df, _ in got] == [(t, tf, df) for t, tf, df, _ in rows], (ctx, list(got), rows)
    assert [bits(s) for _, _, _, s in got] == [bits(w) for _, _, _, w in rows], (ctx, list(got), rows)
    assert got.matches == matches, (ctx, got.matches, matches)


def check_results(got, want, ctx):
    """a result list against [(doc id, score)]: ids, order, score bits"""
    assert not isinstance(got, Exception), (ctx, got)
    assert [d for d, _ in got] == [d for d, _ in want], (ctx, list(got)[:5], want[:5])
    assert [bits(s) for _, s in got] == [bits(s) for _, s in want], ctx
