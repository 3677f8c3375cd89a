"""GPU tier (`-m gpu`) for the total match count: params "total" -> nxs_resp_total.

Truth is the CPU oracle with the limit lifted: total(q) = len(oracle.search(q, limit=doc_count)).
Every check also demands that the ids and score bits returned WITH the total equal those of the
same call without it, and every query of every list is compared."""
import random
import shutil
import struct

import pytest

import nxsearch_amd as N
import nxsfmt
import oracle_lib as O
from nxsearch_amd import corpus

pytestmark = pytest.mark.gpu

MODES = ("auto", "tile", "req", "scan")       # NXS_GPU_COUNT


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def same_results(got, plain, ctx):
    assert [d for d, _ in got] == [d for d, _ in plain], ctx
    assert [bits(s) for _, s in got] == [bits(s) for _, s in plain], ctx


@pytest.fixture(scope="module")
def nxs(tmp_path_factory):
    h = N.Nxs(str(tmp_path_factory.mktemp("base")))
    yield h
    h.close()


def tile_widths():
    import ctypes as C
    w = (C.c_uint32 * 2)()
    L = N.lib()
    L.nxs_test_count_tile_widths.argtypes = [C.POINTER(C.c_uint32)]
    L.nxs_test_count_tile_widths(w)
    return int(w[0]), int(w[1])


class Truth:
    """The oracle's totals of one index, each computed once."""

    def __init__(self, oidx):
        self.oidx = oidx
        self.memo = {}

    def total(self, q, algo=O.BM25, fuzzymatch=False):
        """-> the total, or the SearchError the query ends in"""
        key = (q, algo, fuzzymatch)
        if key not in self.memo:
            try:
                self.memo[key] = len(self.oidx.search(q, algo=algo, limit=max(self.oidx.doc_count, 1),
                                                      fuzzymatch=fuzzymatch))
            except O.SearchError as e:
                self.memo[key] = e
        return self.memo[key]


def check_batch(gidx, truth, qs, ctx, limit=10, algo=(O.BM25, "BM25"), fuzzymatch=False, plain=None):
    """search_batch(total=True) against the same call without it and the oracle's totals"""
    if plain is None:
        plain = gidx.search_batch(qs, limit=limit, algo=algo[1], fuzzymatch=fuzzymatch)
    got = gidx.search_batch(qs, limit=limit, algo=algo[1], fuzzymatch=fuzzymatch, total=True)
    assert len(got) == len(qs)
    for q, g, p in zip(qs, got, plain):
        want = truth.total(q, algo=algo[0], fuzzymatch=fuzzymatch)
        if isinstance(want, O.SearchError):
            assert isinstance(g, N.NxsError) and g.code == want.code and not hasattr(g, "total"), (ctx, q[:60])
            continue
        assert not hasattr(p, "total"), (ctx, q[:60])
        same_results(g, p, (ctx, q[:60]))
        assert g.total == want, (ctx, q[:60], g.total, want)
        assert len(g) == min(limit, want), (ctx, q[:60])
    return plain


def set_mode(monkeypatch, gidx, mode):
    monkeypatch.setenv("NXS_GPU_COUNT", mode)
    gidx.reconfigure()


def random_query(rng, vocab, nmax):
    q = rng.choice(vocab)
    for _ in range(rng.randint(1, nmax) - 1):
        q += rng.choice([" AND ", " OR ", " AND NOT ", " "]) + rng.choice(vocab)
    return q


# ---- tile edges -------------------------------------------------------------------------------

@pytest.mark.parametrize("size", ["W-1", "W", "W+1", "2W+1"])
@pytest.mark.parametrize("which", [0, 1], ids=["u8", "u32"])
def test_tile_edges(nxs, tmp_path, monkeypatch, which, size):
    """Corpora that end just before, on and just behind a boundary of k_count_tile's LDS tile (both
    widths), with a term in every doc, one in exactly the last doc of a tile and one in the first doc of
    the next; all four kernels' routes agree with the oracle."""
    W = tile_widths()[which]
    n = {"W-1": W - 1, "W": W, "W+1": W + 1, "2W+1": 2 * W + 1}[size]
    rng = random.Random(1000 * which + n)
    vocab = ["v%d" % i for i in range(12)]
    docs, did = [], 0
    for i in range(n):
        did += rng.randint(1, 1000)                     # sparse u64 ids
        toks = [rng.choice(vocab) for _ in range(rng.randint(1, 3))] + ["all"]
        if i == W - 1:
            toks.append("last")                         # the last doc of the first tile
        if i == W:
            toks.append("first")                        # the first doc of the next
        if i == n - 1:
            toks.append("tail")
        docs.append((did, toks))
    t, d, _ = nxsfmt.write_index(str(tmp_path), "edge", docs)
    gidx, truth = nxs.open_files(t, d), Truth(O.Index(t, d))
    qs = [random_query(rng, vocab, 6) for _ in range(40)]
    qs += ["all", "last", "first", "tail", "last OR first", "last AND first", "all AND last", "all AND first",
           "all AND NOT last", "all AND NOT first", "last first tail", "all AND tail", "v0 AND NOT all",
           "(last OR first) AND all", "v1 OR last", "first AND NOT v1"]
    # more than eight tokens: word masks and the postfix program
    qs += [" OR ".join(vocab[:9]), " OR ".join(vocab) + " OR last", "(" + " OR ".join(vocab[:10]) + ") AND NOT first",
           " ".join(vocab[2:12]) + " AND all", "(" + " OR ".join(vocab[:9]) + ") AND (last OR first OR tail)"]
    plain = None
    for mode in MODES:
        set_mode(monkeypatch, gidx, mode)
        plain = check_batch(gidx, truth, qs, (size, W, mode), plain=plain)
    assert truth.total("all") == n and truth.total("last") == (1 if n >= W else 0)
    assert truth.total("first") == (1 if n > W else 0)
    gidx.close()


def test_many_tiles_and_driver_windows(nxs, tmp_path, monkeypatch):
    """300 000 docs: dozens of k_count_tile's ranges per query, k_count_req's driver lists span several
    windows, and `auto` mixes the driver kernel with the exact path's count pass in one batch."""
    c = corpus.write_corpus(str(tmp_path), 300_000, 12_000, seed=83)
    terms = corpus.term_strings(12_000, seed=83)
    gidx, truth = nxs.open_files(c["terms"], c["dtmap"]), Truth(O.Index(c["terms"], c["dtmap"]))
    T = lambda r: terms[r - 1].decode()
    qs = corpus.queries_bool5(terms, 12, seed=5, hi=600)
    qs += [" OR ".join(T(r) for r in range(30, 40)), "(%s) AND NOT %s" % (" OR ".join(T(r) for r in range(50, 62)), T(3)),
           "%s AND %s" % (T(1), T(2)), "%s AND NOT %s" % (T(4), T(2)), "%s OR %s" % (T(9000), T(11000)), T(7)]
    plain = None
    for mode in MODES:
        set_mode(monkeypatch, gidx, mode)
        plain = check_batch(gidx, truth, qs, mode, plain=plain)
    gidx.close()


# ---- token counts -----------------------------------------------------------------------------

def random_corpus(rng, n_docs, vocab, max_len=12):
    docs, did = [], 0
    for _ in range(n_docs):
        did += rng.randint(1, 1000)
        docs.append((did, [rng.choice(vocab) for _ in range(rng.randint(1, max_len))]))
    return docs


def test_token_counts_programs_and_wide_plans(nxs, tmp_path, monkeypatch):
    """9 / 20 / 32 tokens (word masks + program), a program of more than 256 items, an evaluation stack of
    70 and 33 / 100 tokens (wide plans: k_scanw's count pass), the empty set as an operand, a query that
    resolves to nothing (total 0) and one that does not parse (no response, no total)."""
    rng = random.Random(19)
    vocab = ["t%d" % i for i in range(320)]
    weights = [1.0 / (i + 1) for i in range(len(vocab))]
    pool = rng.choices(vocab, weights, k=8192)
    docs = random_corpus(rng, 6000, pool, max_len=14)
    t, d, _ = nxsfmt.write_index(str(tmp_path), "tok", docs)
    gidx, truth = nxs.open_files(t, d), Truth(O.Index(t, d))
    qs = [" OR ".join(vocab[:9]), " OR ".join(vocab[40:60]), " OR ".join(vocab[:32]),
          "(" + " OR ".join(vocab[:10]) + ") AND (" + " OR ".join(vocab[5:20]) + ") AND NOT " + vocab[3],
          " ".join(vocab[100:132]),
          "(" + " OR ".join(vocab[:16]) + ") AND NOT (" + " OR ".join(vocab[16:32]) + ")",
          # 140 leaves of 20 distinct tokens: > 256 program items, <= 32 tokens
          " OR ".join("(%s AND %s)" % (vocab[i % 20], vocab[(i * 7 + 3) % 20]) for i in range(70)),
          # right-nested: evaluation stack of 70
          "".join("%s OR (" % vocab[i] for i in range(69)) + vocab[69] + ")" * 69,
          " OR ".join(vocab[:33]), " ".join(vocab[:100]),
          "(" + " OR ".join(vocab[:50]) + ") AND (" + " OR ".join(vocab[40:95]) + ") AND NOT " + vocab[3],
          " OR ".join(vocab[:12]) + " OR nosuchterm", vocab[1] + " AND nosuchterm", vocab[1] + " OR nosuchterm",
          vocab[1] + " AND NOT nosuchterm", " OR ".join(vocab[:35]) + " OR nosuchterm",
          "nosuchterm OR neitherthis", "nosuchterm",
          "broken AND", vocab[0], vocab[0] + " AND " + vocab[1]]
    plain = None
    for mode in MODES:
        set_mode(monkeypatch, gidx, mode)
        plain = check_batch(gidx, truth, qs, mode, plain=plain)
    got = gidx.search_batch(qs, limit=10, fuzzymatch=False, total=True)
    assert got[-4].total == 0 and got[-4] == [] and got[-5].total == 0 and got[-5] == []
    assert isinstance(got[-3], N.NxsError) and not hasattr(got[-3], "total")
    with pytest.raises(N.NxsError):
        gidx.search("broken AND", fuzzymatch=False, total=True)
    gidx.close()


def test_two_slots_naming_one_term(nxs, tmp_path, monkeypatch):
    """Q6: strings that fuzzy-resolve to the SAME term stay two tokens; both slots get their bit."""
    rng = random.Random(23)
    vocab = ["linux", "unix", "erlang", "python", "kernel", "shell", "driver", "thread"]
    docs = random_corpus(rng, 5000, vocab + ["pad%d" % i for i in range(30)], max_len=9)
    t, d, _ = nxsfmt.write_index(str(tmp_path), "dup", docs)
    gidx, truth = nxs.open_files(t, d), Truth(O.Index(t, d))
    qs = ["linus OR linuz", "linus AND linuz AND kernel", "linux AND linus AND NOT shell",
          "linus AND linuz", "linus linuz linvx", "(linus OR erlang) AND linuz", "linus AND NOT linuz"]
    plain = None
    for mode in MODES:
        set_mode(monkeypatch, gidx, mode)
        plain = check_batch(gidx, truth, qs, mode, fuzzymatch=True, plain=plain)
    assert truth.total("linus OR linuz", fuzzymatch=True) == truth.total("linux") > 0
    gidx.close()


# ---- limit and ranking function ------------------------------------------------------------------

def test_total_does_not_depend_on_limit_or_algo(nxs, tmp_path, monkeypatch):
    """The same total at every limit (8001: the exact two-pass path, whose own count pass delivers it) and
    under both ranking functions -- on a corpus with dense terms and TF-IDF outlier lists, where the scans
    of dropped tokens read rewritten posting ranges: the count must not."""
    monkeypatch.setenv("NXS_GPU_DROP_MINPOST", "1")
    monkeypatch.setenv("NXS_GPU_OUTL_SHARE", "64")
    c = corpus.write_corpus(str(tmp_path), 60_000, 4000, seed=83)
    terms = corpus.term_strings(4000, seed=83)
    gidx, truth = nxs.open_files(c["terms"], c["dtmap"]), Truth(O.Index(c["terms"], c["dtmap"]))
    rng = random.Random(3)
    T = lambda r: terms[r - 1].decode()
    qs = []
    for _ in range(12):                                  # dense + sparse pure OR: the dropped-token class
        ranks = rng.sample(range(1, 25), rng.randint(1, 2)) + rng.sample(range(40, 2000), rng.randint(1, 4))
        rng.shuffle(ranks)
        qs.append(" OR ".join(T(r) for r in ranks))
    qs += corpus.queries_bool5(terms, 8, seed=5, hi=400) + [T(1), T(300), "%s AND NOT %s" % (T(2), T(5)),
                                                            "%s OR %s" % (T(1), T(3900))]
    for algo in ((O.BM25, "BM25"), (O.TF_IDF, "TF-IDF")):
        for limit in (1, 10, 64, 65, 1000, 8001):
            check_batch(gidx, truth, qs, (algo[1], limit), limit=limit, algo=algo)
    for q in qs:
        assert truth.total(q, algo=O.BM25) == truth.total(q, algo=O.TF_IDF), q
    # the single-query entry point, default limit
    g = gidx.search(qs[0], fuzzymatch=False, total=True)
    same_results(g, gidx.search(qs[0], fuzzymatch=False), qs[0])
    assert g.total == truth.total(qs[0])
    gidx.close()


def test_ranking_function_that_scores_nothing(nxs, tmp_path):
    """A header with fewer tokens than docs (adl < 1, ranking.c:163-166): BM25 scores nothing -- results and
    total are empty / 0; TF-IDF counts normally."""
    rng = random.Random(5)
    vocab = ["a%d" % i for i in range(9)]
    docs = random_corpus(rng, 700, vocab, max_len=3)
    timg, _, term_ids = nxsfmt.build_images(docs)
    blocks = []
    for did, toks in docs:
        cnt = {}
        for w in toks:
            cnt[term_ids[w.encode()]] = cnt.get(term_ids[w.encode()], 0) + 1
        blocks.append((did, len(toks), sorted(cnt.items())))
    tp, dp = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(tp, "wb").write(timg)
    open(dp, "wb").write(nxsfmt.dtmap_image(blocks, len(docs) - 1, len(docs)))     # token_count < doc_count
    gidx, truth = nxs.open_files(tp, dp), Truth(O.Index(tp, dp))
    qs = ["a0", "a0 OR a1", "a0 AND a1", "a1 AND NOT a2", " OR ".join(vocab)]
    check_batch(gidx, truth, qs, "bm25", algo=(O.BM25, "BM25"))
    check_batch(gidx, truth, qs, "tfidf", algo=(O.TF_IDF, "TF-IDF"))
    for q in qs:
        assert truth.total(q, algo=O.BM25) == 0
    assert truth.total("a0 OR a1", algo=O.TF_IDF) > 0
    got = gidx.search_batch(qs, limit=8001, algo="BM25", fuzzymatch=False, total=True)
    assert [g.total for g in got] == [0] * len(qs) and all(g == [] for g in got)
    gidx.close()


# ---- JSON ---------------------------------------------------------------------------------------

def test_json_member_and_accessor(nxs, tmp_path):
    rng = random.Random(7)
    vocab = ["j%d" % i for i in range(6)]
    t, d, _ = nxsfmt.write_index(str(tmp_path), "js", random_corpus(rng, 400, vocab, max_len=4))
    gidx, oidx = nxs.open_files(t, d), O.Index(t, d)
    q = "j0 OR j1"
    m = len(oidx.search(q, limit=oidx.doc_count))
    assert m > 3
    with_total = gidx.search(q, json=True, params_json='{"limit":3,"total":true}')
    without = gidx.search(q, json=True, params_json='{"limit":3}')
    assert with_total.endswith('],"count":3,"total":%d}' % m)
    assert without == O.results_json(oidx.search(q, limit=3))      # today's text, byte for byte
    assert with_total == without[:-1] + ',"total":%d}' % m
    assert gidx.search(q, json=True, params_json='{"limit":3,"total":false}') == without
    # nxs_resp_total() says false for a response that did not ask: the binding then returns a plain list
    assert not hasattr(gidx.search(q, limit=3), "total")
    assert not hasattr(gidx.search(q, params_json='{"limit":3,"total":false}'), "total")
    assert gidx.search(q, params_json='{"limit":3,"total":true}').total == m
    gidx.close()


# ---- pipelining ------------------------------------------------------------------------------------

def test_pipelined_batches_mixing_total_on_and_off(nxs, tmp_path):
    """Eight batches of 64 queries, four in flight, every other one asking for totals; a quarter of the
    tokens misspelt, so that the batches' fuzzy halves finish late (in the next _begin or the batch's own
    _end).  Totals and results per batch equal the blocking call's and the oracle's."""
    c = corpus.write_corpus(str(tmp_path), 30_000, 2000, seed=47)
    terms = corpus.term_strings(2000, seed=47)
    gidx, truth = nxs.open_files(c["terms"], c["dtmap"]), Truth(O.Index(c["terms"], c["dtmap"]))
    rng = random.Random(11)
    have = set(terms)
    qs = []
    for q in corpus.queries_bool5(terms, 384, seed=13, hi=300) + corpus.queries_single(terms, 128, seed=14, lo=1, hi=300):
        parts = q.split(" ")
        for j, p in enumerate(parts):
            if p not in ("AND", "OR") and rng.random() < 0.25:
                while True:
                    b = bytearray(p.encode())
                    b[rng.randrange(len(b))] = ord("a") + rng.randrange(26)
                    if bytes(b) not in have:
                        break
                parts[j] = bytes(b).decode()
        qs.append(" ".join(parts))
    rng.shuffle(qs)
    batches = [qs[i * 64:(i + 1) * 64] for i in range(8)]
    blocking = [gidx.search_batch(b, limit=10, total=(i % 2 == 0)) for i, b in enumerate(batches)]

    def check(i, got):
        assert len(got) == 64
        for q, g, w in zip(batches[i], got, blocking[i]):
            same_results(g, w, (i, q))
            if i % 2 == 0:
                assert g.total == w.total == truth.total(q, fuzzymatch=True), (i, q, g.total, w.total)
            else:
                assert not hasattr(g, "total") and not hasattr(w, "total"), (i, q)
    inflight = []
    for i, b in enumerate(batches):
        gidx.search_batch_begin(b, limit=10, total=(i % 2 == 0))
        inflight.append(i)
        if len(inflight) == 4:
            check(inflight.pop(0), gidx.search_batch_end())
    while inflight:
        check(inflight.pop(0), gidx.search_batch_end())
    hp = gidx.host_profile()
    assert hp["fuzzy_launch_ms"] > 0, hp               # the late halves did run
    gidx.close()


# ---- refresh -----------------------------------------------------------------------------------------

def test_totals_follow_a_refresh_and_belong_to_their_snapshot(nxs, tmp_path):
    ev = [("add", 10 * (i + 1), ["cat", "dog", "w%d" % (i % 7)] + (["owl"] if i % 3 == 0 else [])) for i in range(900)]
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    t, d = str(tmp_path / "nxsterms"), str(tmp_path / "nxsdtmap")
    open(t, "wb").write(timg + b"\0" * 262144)
    open(d, "wb").write(dimg + b"\0" * 262144)
    gidx = nxs.open_files(t, d)
    qs = ["cat", "owl", "emu", "dog OR emu", "w3 AND cat", "emu AND cat", "owl AND NOT w3", "cat AND NOT owl",
          "w1 OR w2 OR owl", "gnu"]
    snaps = []

    def snapshot():                                     # (a private copy: the oracle reads the header live)
        k = len(snaps)
        tt, dd = str(tmp_path / ("t%d" % k)), str(tmp_path / ("d%d" % k))
        shutil.copy(t, tt)
        shutil.copy(d, dd)
        snaps.append(Truth(O.Index(tt, dd)))
        return snaps[-1]

    def publish():
        timg, dimg, _ = nxsfmt.build_images_log(ev)
        nxsfmt.publish_in_place(t, d, timg, dimg)
        return snapshot()
    check_batch(gidx, snapshot(), qs, "snapshot 0")
    ev.append(("add", 20000, ["cat", "emu", "owl"]))    # an append with a new term
    check_batch(gidx, publish(), qs, "append")
    ev.append(("rm", 30))                               # removals: an old doc and the appended one's neighbour
    ev.append(("rm", 9000))
    check_batch(gidx, publish(), qs, "removal")
    assert snaps[2].total("cat") == snaps[1].total("cat") - 2 and snaps[1].total("emu") == 1
    # a batch begun before the publish: the old snapshot's totals, together with the old results
    gidx.search_batch_begin(qs, limit=10, fuzzymatch=False, total=True)
    ev.append(("add", 20001, ["gnu", "cat", "cat"]))
    ev.append(("rm", 20000))
    new = publish()
    gidx.search_batch_begin(qs, limit=10, fuzzymatch=False, total=True)
    for want, ctx in ((snaps[2], "begun before the publish"), (new, "begun after it")):
        for q, g in zip(qs, gidx.search_batch_end()):
            w = want.oidx.search(q, limit=10, fuzzymatch=False)
            same_results(g, w, (ctx, q))
            assert g.total == want.total(q), (ctx, q, g.total)
    assert snaps[2].total("gnu") == 0 and new.total("gnu") == 1 and new.total("emu") == 0
    gidx.close()


# ---- doc shards ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_shards", [2, 3])
def test_doc_shards_sum_their_totals(nxs, tmp_path, n_shards):
    rng = random.Random(61 + n_shards)
    vocab = ["w%d" % i for i in range(50)]
    weights = [1.0 / (i + 1) for i in range(len(vocab))]
    pool = rng.choices(vocab, weights, k=4096)
    docs = random_corpus(rng, 9000, pool, max_len=7)
    t, d, _ = nxsfmt.write_index(str(tmp_path), "whole", docs)
    truth = Truth(O.Index(t, d))
    shards = [nxs.open_shard(t, d, s_, n_shards) for s_ in range(n_shards)]
    qs = [random_query(rng, vocab[:16], 5) for _ in range(50)]
    qs += ["w0", "w0 AND w1", "w49 OR w0", "w3 OR w4 OR w5 OR w6 OR w7", "broken AND", "w1 AND NOT w0",
           "zzzz OR yyyy", "w2 OR ww3", " OR ".join(vocab[:20])]
    for limit in (10, 300):
        for algo in ((O.BM25, "BM25"), (O.TF_IDF, "TF-IDF")):
            plain = nxs.docshard_search_batch(shards, qs, limit=limit, algo=algo[1], fuzzymatch=False)
            got = nxs.docshard_search_batch(shards, qs, limit=limit, algo=algo[1], fuzzymatch=False, total=True)
            for q, g, p in zip(qs, got, plain):
                want = truth.total(q, algo=algo[0])
                if isinstance(want, O.SearchError):
                    assert isinstance(g, N.NxsError) and g.code == want.code, q
                    continue
                assert not hasattr(p, "total")
                same_results(g, p, (n_shards, q, limit))
                assert g.total == want, (n_shards, q, limit, algo[1], g.total, want)
    for s_ in shards:
        s_.close()


# ---- refusals ------------------------------------------------------------------------------------------

def test_emulated_ranks_refuse_totals(nxs, tmp_path):
    """An emulated world of two ranks: -1 and NXS_ERR_INVALID with "total"; the same call without the key
    still works, and so does "total" once the emulation is off."""
    from nxsearch_amd import multi
    c = corpus.write_corpus(str(tmp_path), 20_000, 1500, seed=73)
    terms = corpus.term_strings(1500, seed=73)
    qs = corpus.queries_bool5(terms, 12, seed=5, hi=300)
    gidx, oidx = nxs.open_files(c["terms"], c["dtmap"]), O.Index(c["terms"], c["dtmap"])
    multi.emulate(gidx, 0, 2)
    with pytest.raises(N.NxsError) as e:
        gidx.search_batch(qs, limit=10, fuzzymatch=False, total=True)
    assert e.value.code == 3 and "total is not available on a sharded batch" in e.value.msg
    with pytest.raises(N.NxsError) as e:
        gidx.search_batch_begin(qs, limit=10, fuzzymatch=False, total=True)
    assert e.value.code == 3
    got = gidx.search_batch(qs, limit=10, fuzzymatch=False)          # (emulation hands out the block only)
    assert len(got) == len(qs) and len(multi.emulated_block(gidx)) == multi.block_bytes(multi.shard_capacity(len(qs), 2), 10)
    multi.emulate(gidx, 0, 0)
    for q, g in zip(qs, gidx.search_batch(qs, limit=10, fuzzymatch=False, total=True)):
        assert g.total == len(oidx.search(q, limit=oidx.doc_count, fuzzymatch=False)), q
    gidx.close()


def test_rank_form_and_communicator_refuse_totals(nxs, tmp_path):
    """The doc shards' rank form on a real RCCL communicator (world 1), and a batch on an index with a
    communicator attached: refused with "total", served without; one query (never sharded) is served."""
    c = corpus.write_corpus(str(tmp_path), 20_000, 1500, seed=73)
    terms = corpus.term_strings(1500, seed=73)
    qs = corpus.queries_bool5(terms, 12, seed=5, hi=300)
    oidx = O.Index(c["terms"], c["dtmap"])
    sh = nxs.open_shard(c["terms"], c["dtmap"], 0, 1)
    sh.shard(0, 1, nxs.shard_unique_id())
    nxs.docshard_attach(sh)
    with pytest.raises(N.NxsError) as e:
        nxs.docshard_search_batch_rank(sh, qs, limit=10, fuzzymatch=False, total=True)
    assert e.value.code == 3 and "total is not available on a sharded batch" in e.value.msg
    for q, g in zip(qs, nxs.docshard_search_batch_rank(sh, qs, limit=10, fuzzymatch=False)):
        same_results(g, oidx.search(q, limit=10, fuzzymatch=False), q)
    with pytest.raises(N.NxsError) as e:
        sh.search_batch(qs, limit=10, fuzzymatch=False, total=True)
    assert e.value.code == 3
    g = sh.search(qs[1], limit=10, fuzzymatch=False, total=True)
    same_results(g, oidx.search(qs[1], limit=10, fuzzymatch=False), qs[1])
    assert g.total == len(oidx.search(qs[1], limit=oidx.doc_count, fuzzymatch=False))
    sh.close()
