"""Truth for the search-within-a-doc-set tests, from the unchanged CPU oracle.

all = oracle.search(q, algo, limit=1 << 20) is R, every result of the query with its score.  The docs of S are kept,
sorted by doc id descending -- the order results.c feeds the heap in -- and put through oracle_lib.topk at the limit:
the reference's capped heap and heap_sort.  Total = the number kept.  Everything is compared in full: ids, order,
score bits, total, and explanations through explain_truth.check."""
import explain_truth
import oracle_lib as O
from explain_truth import Truth as ExTruth, bits, tf_of_docs

UNBOUNDED = 1 << 20


class Truth:
    """One snapshot: docs [(id, [token, ...])] as handed to nxsfmt, the removed ids."""

    def __init__(self, oidx, docs, removed=()):
        self.oidx = oidx
        self.ex = ExTruth(oidx, tf_of_docs(docs, removed))
        self.live = sorted(set(d for d, _ in docs) - set(removed))
        self.memo = {}

    def all(self, q, algo, fuzzymatch=False):
        """R as the oracle returns it (raises oracle_lib.SearchError for a query the oracle rejects)"""
        key = (q, algo, fuzzymatch)
        if key not in self.memo:
            try:
                self.memo[key] = self.oidx.search(q, algo=algo, limit=UNBOUNDED, fuzzymatch=fuzzymatch)
            except O.SearchError as e:
                self.memo[key] = e
        if isinstance(self.memo[key], Exception):
            raise self.memo[key]
        return self.memo[key]

    def kept(self, q, algo, S, fuzzymatch=False):
        """R n S in feed order: descending doc id"""
        S = S if isinstance(S, (set, frozenset)) else set(S)
        return sorted(((d, s) for d, s in self.all(q, algo, fuzzymatch) if d in S), key=lambda x: -x[0])

    def search_docs(self, q, algo, limit, S, fuzzymatch=False, rewritten=None):
        """-> ([(doc, score)] as the reference's heap leaves them, total).  rewritten: the query the oracle runs
        where it is not the string's own (prefix and wildcard leaves)"""
        kept = self.kept(rewritten or q, algo, S, fuzzymatch)
        return O.topk([d for d, _ in kept], [s for _, s in kept], limit), len(kept)


def check_docs(got, want, ctx, total=True):
    """an Index.search_docs entry against Truth.search_docs: ids, order, score bits, total"""
    rows, n = want
    assert not isinstance(got, Exception), (ctx, got)
    assert [d for d, _ in got] == [d for d, _ in rows], (ctx, list(got)[:12], rows[:12])
    assert [bits(s) for _, s in got] == [bits(s) for _, s in rows], (ctx, list(got)[:12], rows[:12])
    if total:
        assert got.total == n, (ctx, got.total, n)


def check_explain(got, plain, truth, q, algo, fuzzymatch, ctx, tokens=None):
    """the explanations of a search_docs entry: explain_truth.check against the same call without them"""
    return explain_truth.check(got, plain, truth.ex, q, algo, fuzzymatch, ctx, tokens)
