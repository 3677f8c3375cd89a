"""N4 doc-sharded collections that follow the index files: nxs_docshard_refresh()
(all shards in this process) and nxs_docshard_refresh_rank() (one process per
shard; its phases played one rank after another here).  The ground truth after
every change is the whole-index oracle loaded freshly from the files: ids, order
and score bits."""
import ctypes as C
import os
import random
import struct

import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from nxsearch_amd import corpus

gpu = pytest.mark.gpu
FATAL = 1


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def assert_same(got, want, ctx=""):
    assert not isinstance(got, Exception), (ctx, got)
    assert [d for d, _ in got] == [d for d, _ in want], ctx
    assert [bits(s) for _, s in got] == [bits(s) for _, s in want], ctx


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def _stats(idx):
    L = N.lib()
    L.nxs_index_refresh_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    out = (C.c_uint64 * 2)()
    L.nxs_index_refresh_stats(idx._h, out)
    return out[0], out[1]


def _impact_passes(idx):
    L = N.lib()
    L.nxs_test_impact_passes.restype = C.c_uint64
    L.nxs_test_impact_passes.argtypes = [C.c_void_p]
    return L.nxs_test_impact_passes(idx._h)


def _inject(idx, nth=1):
    L = N.lib()
    L.nxs_test_inject_failure.argtypes = [C.c_void_p, C.c_int, C.c_uint]
    L.nxs_test_inject_failure(idx._h, 4, nth)


class LogIndex:
    """An index written from an event log (nxsfmt.build_images_log) into files
    sized once, published in place after every change."""

    def __init__(self, tmp, events, pad_t=1 << 16, pad_d=1 << 18):
        self.events = list(events)
        self.t, self.d = str(tmp / "nxsterms"), str(tmp / "nxsdtmap")
        timg, dimg, _ = nxsfmt.build_images_log(self.events)
        with open(self.t, "wb") as f:
            f.write(timg + b"\0" * pad_t)
        with open(self.d, "wb") as f:
            f.write(dimg + b"\0" * pad_d)

    def publish(self, *evs):
        self.events += evs
        timg, dimg, _ = nxsfmt.build_images_log(self.events)
        for path, img in ((self.t, timg), (self.d, dimg)):
            if os.path.getsize(path) < len(img):        # outgrown: the file grows (mapping too small)
                with open(path, "r+b") as f:
                    f.seek(0, 2)
                    f.write(b"\0" * (len(img) - f.tell() + 4096))
        nxsfmt.publish_in_place(self.t, self.d, timg, dimg)

    def oracle(self):
        return O.Index(self.t, self.d)

    def frozen_oracle(self, tmp):
        """The oracle of the files as they are now, on a copy (an in-place publish
        moves what an oracle on the files themselves reads)."""
        import shutil
        os.makedirs(str(tmp), exist_ok=True)
        t, d = str(tmp / "nxsterms"), str(tmp / "nxsdtmap")
        shutil.copyfile(self.t, t)
        shutil.copyfile(self.d, d)
        return O.Index(t, d)


def _zipf_events(rng, n_docs, vocab, max_len):
    weights = [1.0 / (i + 1) for i in range(len(vocab))]
    mk = lambda: rng.choices(vocab, weights, k=rng.randint(1, max_len))
    return [("add", i + 1, mk()) for i in range(n_docs)], mk


def _check(nxs, shards, oidx, qs, limit, algo, ctx, fuzzymatch=None):
    name, code = ("BM25", 1) if algo else ("TF-IDF", 0)
    got = nxs.docshard_search_batch(shards, qs, limit=limit, algo=name, fuzzymatch=fuzzymatch)
    for q, g in zip(qs, got):
        kw = {} if fuzzymatch is None else {"fuzzymatch": fuzzymatch}
        assert_same(g, oidx.search(q, algo=code, limit=limit, **kw), (ctx, q, limit, name))


@gpu
@pytest.mark.parametrize("n_shards", [2, 3])
def test_docshard_refresh_follows_the_files(nxs, tmp_path, n_shards):
    """60 interleaved appends (some with new terms) and removals spread over every
    shard, each published in place and taken by ONE nxs_docshard_refresh(); every
    answer equals the whole-index oracle loaded freshly -- a df change in one shard
    moves the score bits in all of them.  Every shard's impacts are recomputed
    exactly once per refresh, and every refresh is incremental."""
    rng = random.Random(17 + n_shards)
    vocab = ["w%d" % i for i in range(50)]
    events, mk = _zipf_events(rng, 9000, vocab, 7)       # massive ties
    ix = LogIndex(tmp_path, events)
    shards = [nxs.open_shard(ix.t, ix.d, s, n_shards) for s in range(n_shards)]
    fixed = ["w0", "w1 AND w2", "w3 OR w7 OR w20", "w0 AND NOT w1", "w5 OR w40 OR w49 OR w9 OR w2",
             "w2 AND w4 AND w1", "w3 AND (w0 OR w9) AND w1"]
    _check(nxs, shards, ix.oracle(), fixed, 10, 1, "open")
    alive, next_id, n_new = list(range(1, 9001)), 9001, 0
    passes = [_impact_passes(s) for s in shards]
    for step in range(60):
        if step % 3 == 1:
            # a victim in shard (step % S)'s part of the ids -- shard 0 included
            alive.sort()
            part = (step // 3) % n_shards
            lo, hi = len(alive) * part // n_shards, len(alive) * (part + 1) // n_shards
            victim = alive.pop(rng.randrange(lo, hi))
            ix.publish(("rm", victim))
        else:
            evs = []
            for _ in range(rng.randint(1, 3)):
                toks = mk()
                if rng.random() < 0.4:
                    n_new += 1
                    toks.append("fresh%d" % n_new)
                evs.append(("add", next_id, toks))
                alive.append(next_id)
                next_id += rng.randint(1, 4)
            ix.publish(*evs)
        oidx = ix.oracle()
        assert nxs.docshard_refresh(shards) is True, step
        now = [_impact_passes(s) for s in shards]
        assert [b - a for a, b in zip(passes, now)] == [1] * n_shards, (step, passes, now)
        passes = now
        qs = fixed + (["fresh%d" % n_new, "fresh%d OR w1" % max(1, n_new - 1)] if n_new else [])
        if step % 10 == 0 and n_new:
            qs.append("w0 OR frush%d" % n_new)      # fuzzy -> the newest term
        _check(nxs, shards, oidx, qs, (10, 64, 1000)[step % 3], step % 2, step)
    assert [_stats(s) for s in shards] == [(60, 0)] * n_shards
    assert nxs.docshard_refresh(shards) is False

    # a synthetic corpus: sparse and dense terms; docs appended and removed in the raw files
    c = corpus.write_corpus(str(tmp_path / "syn"), 40_000, 3000, seed=29)
    terms = corpus.term_strings(3000, seed=29)
    sh2 = [nxs.open_shard(c["terms"], c["dtmap"], s, n_shards) for s in range(n_shards)]
    raw = RawFiles(c["terms"], c["dtmap"])
    qs = corpus.queries_bool5(terms, 24, seed=5, hi=300) + corpus.queries_single(terms, 6, seed=6, lo=1, hi=100)
    ids = sorted(raw.blocks)
    for step in range(8):
        if step % 2:
            part = step % n_shards
            victim = ids.pop(rng.randrange(len(ids) * part // n_shards, len(ids) * (part + 1) // n_shards))
            raw.remove(victim)
        else:
            word = b"newterm%d" % step
            tid = raw.append_term(word)
            raw.append_doc(50_000 + step, [(tid, 2), (1, 1), (rng.randint(2, 300), 1)])
            qs.append(word.decode())
        assert nxs.docshard_refresh(sh2) is True
        _check(nxs, sh2, O.Index(c["terms"], c["dtmap"]), qs, (10, 1000)[step % 2], step % 2, ("syn", step),
               fuzzymatch=False)
    for s in shards + sh2:
        s.close()


class RawFiles:
    """Appends to and removals from an index written by corpus.write_corpus, the way
    an indexer process changes the files: block first, header last."""

    def __init__(self, tpath, dpath):
        self.t, self.d = tpath, dpath
        self.blocks = {}
        with open(dpath, "rb") as f:
            img = f.read()
        data_len = struct.unpack(">Q", img[8:16])[0]
        off = 0
        while off < data_len:
            doc_id, doc_len, np_ = struct.unpack(">QII", img[32 + off:48 + off])
            if doc_id and doc_len:
                self.blocks[doc_id] = (32 + off, doc_len)
            off += 16 + 8 * np_
        with open(tpath, "rb") as f:
            timg = f.read()
        t_len, off, self.n_terms = struct.unpack(">I", timg[8:12])[0], 0, 0
        while off < t_len:
            ln = struct.unpack(">H", timg[16 + off:18 + off])[0]
            off += ((2 + ln + 1 + 7) & ~7) + 8
            self.n_terms += 1

    def _hdr(self, f):
        f.seek(8)
        return struct.unpack(">QQI", f.read(20))

    def append_doc(self, doc_id, pairs):
        with open(self.d, "r+b") as f:
            data_len, tokens, docs = self._hdr(f)
            n = sum(c for _, c in pairs)
            blk = struct.pack(">QII", doc_id, n, len(pairs)) + b"".join(struct.pack(">II", t, c) for t, c in sorted(pairs))
            f.seek(32 + data_len)
            f.write(blk)
            f.flush()
            f.seek(8)
            f.write(struct.pack(">QQI", data_len + len(blk), tokens + n, docs + 1))
        self.blocks[doc_id] = (32 + data_len, n)

    def remove(self, doc_id):
        off, doc_len = self.blocks.pop(doc_id)
        with open(self.d, "r+b") as f:
            data_len, tokens, docs = self._hdr(f)
            f.seek(off)
            f.write(struct.pack(">Q", 0))
            f.seek(32 + data_len)
            f.write(struct.pack(">QII", doc_id, 0, 0))
            f.flush()
            f.seek(8)
            f.write(struct.pack(">QQI", data_len + 16, tokens - doc_len, docs - 1))

    def append_term(self, word):
        with open(self.t, "r+b") as f:
            f.seek(8)
            data_len = struct.unpack(">I", f.read(4))[0]
            blk = struct.pack(">H", len(word)) + word + b"\0"
            blk += b"\0" * (-len(blk) % 8) + struct.pack(">Q", 2)
            f.seek(16 + data_len)
            f.write(blk)
            f.flush()
            f.seek(8)
            f.write(struct.pack(">I", data_len + len(blk)))
        self.n_terms += 1
        return self.n_terms


@gpu
def test_docshard_static_until_refreshed(nxs, tmp_path):
    """A publish is not seen before the refresh (the shards serve the old snapshot);
    a second refresh with nothing new returns False."""
    rng = random.Random(5)
    events, mk = _zipf_events(rng, 3000, ["w%d" % i for i in range(30)], 6)
    ix = LogIndex(tmp_path, events)
    shards = [nxs.open_shard(ix.t, ix.d, s, 2) for s in range(2)]
    qs = ["w0", "w1 OR w2", "w3 AND w4", "w0 OR novel"]
    assert nxs.docshard_refresh(shards) is False
    before = ix.frozen_oracle(tmp_path / "before")
    ix.publish(("add", 5000, ["w0", "novel", "w0"]), ("rm", 17), ("rm", 2900))
    _check(nxs, shards, before, qs, 10, 1, "stale", fuzzymatch=False)
    assert nxs.docshard_refresh(shards) is True
    _check(nxs, shards, ix.oracle(), qs, 10, 1, "fresh", fuzzymatch=False)
    assert nxs.docshard_refresh(shards) is False
    for s in shards:
        s.close()


@gpu
def test_docshard_refresh_full_rebuild(nxs, tmp_path):
    """A removed id that comes back, an id below the maximum, files that outgrow
    their mapping: every shard rebuilds its slice of the agreed snapshot; exact."""
    rng = random.Random(7)
    events, mk = _zipf_events(rng, 4000, ["w%d" % i for i in range(40)], 6)
    ix = LogIndex(tmp_path, events, pad_t=64, pad_d=64)
    shards = [nxs.open_shard(ix.t, ix.d, s, 3) for s in range(3)]
    qs = ["w0", "w1 OR w2", "w3 AND w4", "w5 OR w30 OR back", "w0 AND NOT w1"]
    ix.publish(("rm", 10), ("rm", 2500))
    assert nxs.docshard_refresh(shards) is True
    _check(nxs, shards, ix.oracle(), qs, 64, 1, "removed")
    ix.publish(("add", 10, ["w0", "back", "w2"]))            # a removed id comes back
    assert nxs.docshard_refresh(shards) is True
    _check(nxs, shards, ix.oracle(), qs, 64, 0, "re-used id")
    assert [_stats(s)[1] for s in shards] == [1, 1, 1]
    ix.publish(("add", 4500, ["w1"]), ("add", 4200, ["w1", "back"]))
    assert nxs.docshard_refresh(shards) is True                 # 4200 < 4500: out of order
    _check(nxs, shards, ix.oracle(), qs, 1000, 1, "out of order")
    assert [_stats(s)[1] for s in shards] == [2, 2, 2]
    # 3000 more docs: both files grow past their mapping (remapped), new terms
    ix.publish(*[("add", 10_000 + i, [mk()[0], "t%d" % (i // 3)]) for i in range(3000)])
    assert nxs.docshard_refresh(shards) is True
    _check(nxs, shards, ix.oracle(), qs + ["t999", "t5 OR t7"], 1000, 0, "grown")
    for s in shards:
        s.close()


@gpu
def test_docshard_refresh_rank_form_emulated(nxs, tmp_path):
    """The rank protocol with the ranks played one after the other: rank 1 reads a
    later snapshot than rank 0 (a publish in between) -- every rank consumes to the
    later one.  An injected failure of one rank's device step makes every rank
    return -1 and refuse searches (NXS_ERR_FATAL) until the next refresh rebuilds."""
    rng = random.Random(11)
    events, mk = _zipf_events(rng, 5000, ["w%d" % i for i in range(40)], 7)
    ix = LogIndex(tmp_path, events)
    shards = [nxs.open_shard(ix.t, ix.d, s, 2) for s in range(2)]
    qs = ["w0", "w1 AND w2", "w3 OR w7 OR w20", "late", "w0 OR late", "early OR w9"]
    ix.publish(("add", 6000, ["w0", "early"]), ("rm", 3))
    later = [("add", 6001, ["late", "w1", "w2"]), ("rm", 4000), ("add", 6005, ["late", "w0"])]
    rets = nxs.docshard_emulated_refresh(shards, after_record=lambda r: r == 0 and ix.publish(*later))
    assert rets == [1, 1]
    oidx = ix.oracle()
    _check(nxs, shards, oidx, qs, 10, 1, "later snapshot", fuzzymatch=False)
    for per_rank in nxs.docshard_emulated_ranks(shards, qs, limit=64, fuzzymatch=False):
        for q, g in zip(qs, per_rank):
            assert_same(g, oidx.search(q, limit=64, fuzzymatch=False), ("rank form", q))
    assert nxs.docshard_emulated_refresh(shards) == [0, 0]
    # rank 1's device step fails after rank 0 merged
    ix.publish(("add", 6100, ["w3", "late"]), ("rm", 100))
    _inject(shards[1])
    assert nxs.docshard_emulated_refresh(shards) == [-1, -1]
    with pytest.raises(N.NxsError) as e:
        nxs.docshard_search_batch(shards, qs, limit=10)
    assert e.value.code == FATAL
    rb = [_stats(s)[1] for s in shards]
    assert nxs.docshard_emulated_refresh(shards) == [1, 1]
    assert [_stats(s)[1] for s in shards] == [x + 1 for x in rb]
    _check(nxs, shards, ix.oracle(), qs, 10, 0, "after the failure", fuzzymatch=False)
    # the in-process form likewise
    ix.publish(("add", 6200, ["w4", "late"]))
    _inject(shards[0])
    with pytest.raises(N.NxsError):
        nxs.docshard_refresh(shards)
    with pytest.raises(N.NxsError) as e:
        nxs.docshard_search_batch(shards, qs, limit=10)
    assert e.value.code == FATAL
    assert nxs.docshard_refresh(shards) is True
    _check(nxs, shards, ix.oracle(), qs, 10, 1, "in-process, after the failure", fuzzymatch=False)
    for s in shards:
        s.close()


@gpu
def test_docshard_refresh_rank_through_rccl(nxs, tmp_path):
    """nxs_docshard_refresh_rank() end to end on one rank with a real RCCL communicator."""
    from nxsearch_amd import multi
    rng = random.Random(13)
    events, mk = _zipf_events(rng, 4000, ["w%d" % i for i in range(40)], 7)
    ix = LogIndex(tmp_path, events)
    sh = nxs.open_shard(ix.t, ix.d, 0, 1)
    multi.attach(nxs, sh, 0, 1)
    nxs.docshard_attach(sh)
    qs = ["w0", "w1 AND w2", "w3 OR w7 OR w20", "brandnew OR w5"]
    ix.publish(("add", 5000, ["brandnew", "w5"]), ("rm", 1), ("rm", 3999))
    assert nxs.docshard_refresh_rank(sh) is True
    oidx = ix.oracle()
    for q, g in zip(qs, nxs.docshard_search_batch_rank(sh, qs, limit=10, fuzzymatch=False)):
        assert_same(g, oidx.search(q, limit=10, fuzzymatch=False), q)
    assert nxs.docshard_refresh_rank(sh) is False
    sh.close()


def _agree(recs, consumed):
    L = N.lib()
    u64p = C.POINTER(C.c_uint64)
    L.nxs_test_docshard_agree.argtypes = [u64p, C.c_uint, u64p, u64p]
    flat = (C.c_uint64 * (8 * len(recs)))(*[w for r in recs for w in (list(r) + [0] * 8)[:8]])
    cons = (C.c_uint64 * 4)(*consumed)
    out = (C.c_uint64 * 8)()
    r = L.nxs_test_docshard_agree(flat, len(recs), cons, out)
    return r, list(out)


def test_docshard_snapshot_agreement_rule():
    """Rank protocol step 1 (host only): the record with the largest dtmap length,
    the lowest rank on ties; the collection's highest doc id; a rank that reports a
    failure fails every rank; all records equal to what was consumed = nothing to do;
    a rank marked inconsistent forces a rebuild."""
    # terms, dtmap, docs, tokens, max id, status, rebuild
    cons = [100, 200, 10, 50]
    same = [100, 200, 10, 50, 7, 0, 0]
    assert _agree([same, same, same], cons)[0] == 0
    r, out = _agree([same, [100, 200, 10, 50, 99, 0, 0], same], cons)
    assert r == 0       # (the highest doc id alone is no change)
    r, out = _agree([[120, 260, 11, 55, 5, 0, 0], [130, 260, 12, 56, 9, 0, 0], [110, 240, 11, 54, 3, 0, 0]], cons)
    assert r == 1 and out[:4] == [120, 260, 11, 55] and out[4] == 9 and out[6] == 0      # tie: lowest rank
    r, out = _agree([[110, 240, 11, 54, 3, 0, 0], [130, 300, 12, 56, 9, 0, 0], [140, 290, 13, 57, 1, 0, 0]], cons)
    assert r == 1 and out[:4] == [130, 300, 12, 56] and out[4] == 9
    assert _agree([same, [130, 300, 12, 56, 9, 1, 0], same], cons)[0] == -1          # a rank failed
    assert _agree([[130, 300, 12, 56, 9, 0, 0], same, [0] * 5 + [3, 0]], cons)[0] == -1
    r, out = _agree([same, [100, 200, 10, 50, 7, 0, 1]], cons)
    assert r == 1 and out[6] == 1 and out[:4] == cons                                 # inconsistent: rebuild
    r, out = _agree([[100, 200, 10, 51, 7, 0, 0]], cons)
    assert r == 1 and out[3] == 51                                                    # header counter alone
