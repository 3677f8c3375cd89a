"""Truth for the match_docs tests, from the unchanged CPU oracle.

M = the doc ids of oracle.search(q, algo, limit=1 << 20): every result of the query, that is the doc set "total"
counts.  Sorted ascending, filtered to id >= start, the first `limit` ids are the page; total = |M|; next = the
last id of the page + 1 when a doc of M lies beyond the page, else None.  Ids, count, total and next are compared in
full."""
import oracle_lib as O

UNBOUNDED = 1 << 20


class Truth:
    """One snapshot: docs [(id, [token, ...])] as handed to nxsfmt, the removed ids."""

    def __init__(self, oidx, docs, removed=()):
        self.oidx = oidx
        self.live = sorted(set(d for d, _ in docs) - set(removed))
        self.memo = {}

    def M(self, q, algo=O.BM25, fuzzymatch=False):
        """the doc set, ascending (raises oracle_lib.SearchError for a query the oracle rejects)"""
        key = (q, algo, fuzzymatch)
        if key not in self.memo:
            try:
                self.memo[key] = sorted(d for d, _ in self.oidx.search(q, algo=algo, limit=UNBOUNDED, fuzzymatch=fuzzymatch))
            except O.SearchError as e:
                self.memo[key] = e
        if isinstance(self.memo[key], Exception):
            raise self.memo[key]
        return self.memo[key]

    def page(self, q, algo=O.BM25, limit=1000, start=0, fuzzymatch=False, rewritten=None):
        """-> (ids, total, next).  rewritten: the query the oracle runs where it is not the string's own (prefix and
        wildcard leaves)"""
        return page_of(self.M(rewritten or q, algo, fuzzymatch), limit, start)


def page_of(M, limit, start=0):
    """the page of an ascending doc set"""
    rest = [d for d in M if d >= start]
    ids = rest[:limit]
    return ids, len(M), (ids[-1] + 1 if len(rest) > len(ids) else None)


def check_page(got, want, ctx):
    """an Index.match_docs entry against Truth.page: ids, count, total, next"""
    ids, total, nxt = want
    assert not isinstance(got, Exception), (ctx, got)
    assert len(got) == len(ids) and list(got) == ids, (ctx, list(got)[:12], ids[:12], len(got), len(ids))
    assert got.total == total, (ctx, got.total, total)
    assert got.next == nxt, (ctx, got.next, nxt)
