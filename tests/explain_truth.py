"""Truth for the explanation tests, from the CPU oracle and the docs a test wrote.

For term bytes w, oracle.search(w, algo, limit=doc_count, fuzzymatch=False) on an index without filters is the
map doc -> float of that (term, doc): a one-token query's score is 0 + rank(term, doc).  The docs missing from
it are the absent ones.  The token list of a query is what the reference's query_prepare builds: the leaf
strings right to left, equal strings merged (first seen), each resolved by lookup, then (fuzzymatch) by the
BK-tree walk; unresolved tokens are left out, two strings that resolve to one term stay two tokens.  tf comes
from the docs themselves."""
import re
import struct

import numpy as np

_LEAF = re.compile(r"""[()]|[^\s()]+""")
_OPS = ("AND", "OR", "NOT", "(", ")")


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def tf_of_docs(docs, removed=()):
    """{term bytes: {doc id: tf}} of the docs handed to nxsfmt.write_index"""
    out = {}
    gone = set(removed)
    for did, toks in docs:
        if did in gone:
            continue
        for t in toks:
            t = t.encode() if isinstance(t, str) else t
            m = out.setdefault(t, {})
            m[did] = m.get(did, 0) + 1
    return out


def tf_of_events(ev):
    docs, removed = [], set()
    for e in ev:
        if e[0] == "add":
            docs.append((e[1], e[2]))
        else:
            removed.add(e[1])
    return tf_of_docs(docs, removed)


def tf_of_dtmap(path, terms, wanted):
    """The same from an nxsdtmap file a test wrote through corpus.write_corpus, for the term ids in `wanted`
    (terms: bytes in term-id order): the file's doc blocks are u64 id | u32 len | u32 n | n x (u32 term, u32 tf),
    big-endian, behind a 32-byte header."""
    raw = open(path, "rb").read()
    assert raw[:5] == b"NXS_D"
    body_len = struct.unpack_from(">Q", raw, 8)[0]
    words = np.frombuffer(raw, dtype=">u4", count=body_len // 4, offset=32)
    starts, counts, ids = [], [], []
    at = 0
    while at < len(words):
        did = (int(words[at]) << 32) | int(words[at + 1])
        n = int(words[at + 3])
        if did and int(words[at + 2]):
            starts.append(at + 4)
            counts.append(n)
            ids.append(did)
        at += 4 + 2 * n
    counts = np.asarray(counts)
    base = np.repeat(np.asarray(starts), counts) + 2 * (np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts))
    tid, tf = words[base].astype(np.int64), words[base + 1].astype(np.int64)
    did = np.repeat(np.asarray(ids, dtype=np.uint64), counts)
    out = {}
    for t in wanted:
        m = tid == t
        out[terms[t - 1]] = dict(zip(did[m].tolist(), tf[m].tolist()))
    return out


class Truth:
    """One snapshot: its oracle index and the tf of its docs."""

    def __init__(self, oidx, tf):
        self.oidx, self.tf = oidx, tf
        self.memo, self.tok_memo = {}, {}

    def contrib(self, w, algo):
        """{doc id: the oracle's float of (term w, doc)}, computed once per term and ranking function"""
        key = (w, algo)
        if key not in self.memo:
            self.memo[key] = dict(self.oidx.search(w, algo=algo, limit=max(self.oidx.doc_count, 1), fuzzymatch=False))
        return self.memo[key]

    def tokens(self, q, fuzzymatch):
        """the dictionary terms of the query's token list, in list order"""
        key = (q, fuzzymatch)
        if key not in self.tok_memo:
            leaves = [x for x in _LEAF.findall(q) if x not in _OPS]
            seen, out = [], []
            for s in reversed(leaves):
                s = s.encode()
                if s in seen:
                    continue
                seen.append(s)
                tid = self.oidx.lookup(s)
                if not tid and fuzzymatch:
                    tid = self.oidx.fuzzy(s)[0]
                if tid:
                    out.append(self.oidx.term(tid))
            self.tok_memo[key] = out
        return self.tok_memo[key]


def check(got, plain, truth, q, algo, fuzzymatch, ctx, tokens=None):
    """One result list that asked for explanations against the same call without (a), the truth's token list
    (b), presence (c), contribution bits (d), tf (e) and the f32 sum in ascending j (f).  tokens: the list to
    expect if it is not the query's own (a rewritten query's)."""
    ctx = (ctx, q[:80])
    assert not isinstance(got, Exception) and not isinstance(plain, Exception), ctx
    assert [d for d, _ in got] == [d for d, _ in plain], ctx                                        # (a)
    assert [bits(s) for _, s in got] == [bits(s) for _, s in plain], ctx
    assert getattr(plain, "tokens", None) is None and getattr(plain, "explain", None) is None, ctx
    if not len(got):
        assert got.tokens == [] and got.explain == [], ctx
        return 0
    want = truth.tokens(q, fuzzymatch) if tokens is None else tokens
    assert got.tokens == want, (ctx, got.tokens, want)                                              # (b)
    maps = [truth.contrib(w, algo) for w in want]
    tfs = [truth.tf.get(w, {}) for w in want]
    assert len(got.explain) == len(got), ctx
    for (doc, score), row in zip(got, got.explain):
        present = [j for j in range(len(want)) if doc in maps[j]]
        assert [j for j, _, _ in row] == present, (ctx, doc, row, present)                          # (c)
        acc = np.float32(0.0)
        for j, tf, s in row:
            assert bits(s) == bits(maps[j][doc]), (ctx, doc, j, s, maps[j][doc])                    # (d)
            assert tf == tfs[j].get(doc), (ctx, doc, j, tf, tfs[j].get(doc))                        # (e)
            acc = np.float32(acc + np.float32(s))
        assert bits(float(acc)) == bits(score), (ctx, doc, float(acc), score)                       # (f)
        assert present, (ctx, doc)
    return sum(len(r) for r in got.explain)
