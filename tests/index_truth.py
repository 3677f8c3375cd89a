"""Host model of the device index image, and the corpus the image tests run on.

Plain Python and numpy; no code of the library.  A snapshot is an event log (nxsfmt.build_images_log), the CPU
oracle opened on the files written from it, and the ordinal table: the doc id of every device ordinal.  A
freshly loaded index numbers the live docs in file order; a refresh appends ordinals and keeps the dead ones.

From those the model states what every array of the image must hold:

  canonical postings  per term the (doc id, tf) pairs, ascending by doc id, from the events
  impacts             the oracle's float of every (term, doc): a one-token search at limit = doc_count,
                      fuzzymatch off, is the map doc -> float (as tests/explain_truth.py takes it)
  maximp              the bit pattern of the term's largest positive impact, 0 for an empty row
  blkmap / bmrank     bit (o >> 6) & 63 of word o >> 12 per posting ordinal o; bmrank[e] = the number of
                      postings below ordinal 4096 e, e = 0 .. words
  dense set           df >= 1024 and df > scanm_dens x n_docs (n_docs counts dead ordinals), the 64 largest
                      by df (ties: the lower id), ascending by id
  dense_col           the impact bits at the term's ordinals, 0xffffffff elsewhere
  outlier lists       TF-IDF, per dense term: cap = the smallest tf in 1..61 with #(tf > cap) <= n // outl_share
                      over the tf histogram clamped to 63; no list if nothing lies above it or it reaches 62;
                      the list is (ordinal, f32(imp) - f32(cap_imp)) for tf > cap in list order, cap_imp =
                      f32(log(cap + 1)) * idf as an f32 product, idf = f32(log(double(f32(N) / f32(df))) + 1)
                      with math.log (the host libm the library's tables come from); outl_cap = cap_imp, or
                      maximp without a list; outl_max = the largest excess

ShardModel is the view of one doc shard of such a model: the impacts, N, adl and df_global of the
whole collection, everything structural from the shard's own lists and ordinal table.  check_image compares one
device image (Index.device_image) with either model; image_of makes the image a model stands for.
"""
import math
import struct

import numpy as np

TF_IDF, BM25 = 0, 1
ALGOS = (TF_IDF, BM25)
ABSENT = 0xffffffff


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def bits_f32(b):
    return struct.unpack("<f", struct.pack("<I", b))[0]


# ---------------------------------------------------------------------------------------------------
# pieces that stand alone (the CPU tier runs them on hand-made lists)
# ---------------------------------------------------------------------------------------------------

def blkmap_of(ordinals, words):
    """[words] u64: bit (o >> 6) & 63 of word o >> 12 for every posting ordinal o"""
    bm = [0] * words
    for o in ordinals:
        o = int(o)
        bm[o >> 12] |= 1 << ((o >> 6) & 63)
    return np.array(bm, dtype=np.uint64)


def bmrank_of(ordinals, words):
    """[words + 1] u32: the list position of the first posting at or above ordinal 4096 e"""
    o = np.asarray(ordinals, dtype=np.int64)
    return np.searchsorted(o, 4096 * np.arange(words + 1, dtype=np.int64), side="left").astype(np.uint32)


def outlier_cap(tfs, share):
    """-> (cap or None: no list, how many postings lie above it)"""
    n = len(tfs)
    hist = [0] * 64
    for tf in tfs:
        hist[min(int(tf), 63)] += 1
    above = lambda c: sum(hist[c + 1:])
    cap = next((c for c in range(1, 62) if above(c) <= n // share), 62)
    if cap >= 62 or above(cap) == 0:
        return None, 0
    return cap, above(cap)


def tfidf_idf(n_live, df):
    return np.float32(math.log(float(np.float32(n_live) / np.float32(df))) + 1.0)


def tfidf_cap_imp(cap, n_live, df):
    return np.float32(np.float32(math.log(cap + 1)) * tfidf_idf(n_live, df))


def dense_set(dfs, n_docs, scanm_dens):
    """dfs: {term id: df} -> ascending term ids"""
    dn = [(df, t) for t, df in dfs.items() if df >= 1024 and float(df) > scanm_dens * float(n_docs)]
    dn.sort(key=lambda e: (-e[0], e[1]))
    return sorted(t for _, t in dn[:64])


def bitmap_set(dfs, n_docs, bm_share, use_blkmap=True):
    """the rows rebuild_impacts gives a bitmap: df >= max(1, n_docs // bm_share), the 8192 largest by df"""
    if not use_blkmap:
        return []
    min_df = max(1, n_docs // max(bm_share, 1))
    bt = [(df, t) for t, df in dfs.items() if df >= min_df]
    bt.sort(key=lambda e: (-e[0], e[1]))
    return sorted(t for _, t in bt[:8192])


def q8_bounds(imp_bits, max_bits):
    """[lo, hi] of the byte of a posting: L = ceil(255 imp / max) exactly; max(L, 1) <= q8 <= min(255, L + 1).
    The lower bound is what k_scans<.., DROP> prunes on; the upper one follows from the kernel's arithmetic
    (three f32 roundings and a factor 1.00001 on a value <= 255 add less than 0.0027)."""
    from fractions import Fraction
    mx = Fraction(bits_f32(int(max_bits)))
    memo = {}
    lo = np.empty(len(imp_bits), dtype=np.int64)
    for i, b in enumerate(imp_bits.tolist()):
        if b not in memo:
            memo[b] = math.ceil(255 * Fraction(bits_f32(b)) / mx)
        lo[i] = memo[b]
    return np.maximum(lo, 1), np.minimum(255, lo + 1)


# ---------------------------------------------------------------------------------------------------
# the model of one snapshot
# ---------------------------------------------------------------------------------------------------

def replay(events):
    """-> (terms: bytes in term-id order, docs: {doc id: (doc_len, {term id: tf})} of the live docs, file order
    of every doc ever added)"""
    ids, terms, docs, order = {}, [], {}, []
    for ev in events:
        if ev[0] == "add":
            counts = {}
            for t in ev[2]:
                t = t.encode() if isinstance(t, str) else t
                counts[t] = counts.get(t, 0) + 1
            for t in counts:
                if t not in ids:
                    ids[t] = len(terms) + 1
                    terms.append(t)
            assert ev[1] not in docs
            docs[ev[1]] = (len(ev[2]), {ids[t]: c for t, c in counts.items()})
            order.append(ev[1])
        else:
            del docs[ev[1]]
    return terms, docs, order


class Model:
    """events + oracle + the ordinal table (ord_ids[o] = doc id of ordinal o, dead ones included)."""

    def __init__(self, events, oidx, ord_ids, replayed=None):
        self.terms, self.docs, _ = replayed or replay(events)
        self.n_terms = len(self.terms)
        self.oidx = oidx
        self.doc_count, self.token_count = oidx.doc_count, oidx.token_count     # the files' header counters
        self.ord_ids = np.asarray(ord_ids, dtype=np.uint64)
        self.ord_of = {int(d): o for o, d in enumerate(ord_ids)}
        self.live = np.array([int(d) in self.docs for d in ord_ids], dtype=bool)
        self.n_live = len(self.docs)
        assert self.n_live == int(self.live.sum()), "a live doc without an ordinal"
        # canonical postings: (doc id, tf) ascending by doc id
        rows = {t: [] for t in range(1, self.n_terms + 1)}
        for did in sorted(self.docs):
            for t, c in self.docs[did][1].items():
                rows[t].append((did, c))
        self.canon = rows
        self.df = {t: len(r) for t, r in rows.items()}
        self.ords = {t: np.array([self.ord_of[d] for d, _ in r], dtype=np.int64) for t, r in rows.items()}
        self.tfs = {t: np.array([c for _, c in r], dtype=np.int64) for t, r in rows.items()}
        for t, o in self.ords.items():
            assert (np.diff(o) > 0).all(), "doc ids must ascend with the ordinals"
        self._imp = {}
        # what the statistics of the ranking functions are taken over: this index (a shard view differs)
        self.coll_live, self.coll_df = self.n_live, self.df
        self.coll_tokens = sum(l for l, _ in self.docs.values())

    def df_global(self):
        """the collection-wide df array of a doc shard; None: this index is the collection"""
        return None

    def tid(self, name):
        return self.terms.index(name.encode() if isinstance(name, str) else name) + 1

    def impacts(self, t, algo):
        """u32[df]: the bits of the oracle's float of every posting of term t, in list order"""
        key = (t, algo)
        if key not in self._imp:
            if self.df[t] == 0:
                self._imp[key] = np.zeros(0, dtype=np.uint32)
            else:
                got = dict(self.oidx.search(self.terms[t - 1], algo=algo, limit=max(self.oidx.doc_count, 1),
                                            fuzzymatch=False))
                assert len(got) == self.df[t], (self.terms[t - 1], len(got), self.df[t])
                self._imp[key] = np.array([f32_bits(got[d]) for d, _ in self.canon[t]], dtype=np.uint32)
        return self._imp[key]

    def freeze(self):
        """Ask the oracle for everything now: its index follows files that are rewritten in place."""
        for t in range(1, self.n_terms + 1):
            for algo in ALGOS:
                self.impacts(t, algo)
        self.oidx = None
        return self

    def maximp(self, t, algo):
        """impacts are >= +0, where the order of the bit patterns is the order of the floats"""
        b = self.impacts(t, algo)
        return int(b.max()) if len(b) and bits_f32(int(b.max())) > 0.0 else 0

    def blkmap(self, t, words):
        return blkmap_of(self.ords[t], words)

    def bmrank(self, t, words):
        return bmrank_of(self.ords[t], words)

    def dense_terms(self, n_docs, scanm_dens):
        return dense_set(self.df, n_docs, scanm_dens)

    def bm_terms(self, n_docs, bm_share, use_blkmap=True):
        return bitmap_set(self.df, n_docs, bm_share, use_blkmap)

    def dense_col(self, t, algo, n_docs):
        col = np.full(n_docs, ABSENT, dtype=np.uint32)
        col[self.ords[t]] = self.impacts(t, algo)
        return col

    def outliers(self, t, share):
        """TF-IDF -> (cap tf or None, list ordinals, list excess bits, outl_cap bits, outl_max bits)"""
        cap, _ = outlier_cap(self.tfs[t], share)
        imp = self.impacts(t, TF_IDF)
        if cap is None:
            return None, np.zeros(0, np.int64), np.zeros(0, np.uint32), self.maximp(t, TF_IDF), 0
        cap_imp = tfidf_cap_imp(cap, self.coll_live, self.coll_df[t])
        m = self.tfs[t] > cap
        excess = (imp[m].view(np.float32) - cap_imp).astype(np.float32)
        xb = excess.view(np.uint32)
        assert (excess > 0).all()
        return cap, self.ords[t][m], xb, f32_bits(float(cap_imp)), int(xb.max())


# ---------------------------------------------------------------------------------------------------
# the corpus of the image tests: one log, five snapshots (events[:cut[k]] is snapshot k)
# ---------------------------------------------------------------------------------------------------

N0 = 4 * 4096 + 7               # live docs of snapshot 0
ALL_TF = {100: 40, 5000: 62, 9000: 63, 12000: 64, 16000: 200}
N_FILLER = 300
GHOSTS = ("ghosta", "ghostb", "ghostc")
SEAM = (63, 64, 4095, 4096, 8191, 8192)
RUN = tuple(range(0, 100, 10)) + tuple(range(4000, 4200))      # the run starts at list position 10: its word-0
# part (4000 .. 4095) lies at positions 10 .. 105, across the 64-posting window that ends at 63
D1023 = frozenset(11 + 13 * i for i in range(1023))
D1024 = frozenset(2 + 15 * i for i in range(1024))
D1025 = frozenset(7 + 14 * i for i in range(1025))
FLAT = frozenset(range(3000, 13000, 5))
GAP = frozenset(1000 + 3 * i for i in range(20)) | frozenset(3 * 4096 + 50 + 5 * i for i in range(20))
LATE = frozenset(2 * 4096 + 10 + 100 * i for i in range(30))
RM1 = (0, N0 - 1, 4100, 47)     # snapshot 1: first and last ordinal (the last is `one`'s doc), inside `run`, a d1024 doc
N_APPEND3 = 4100


def doc_id(o):
    """sparse, ascending; above 2^32 from ordinal 9000 on"""
    return 1000 + 16 * o + (o * o) % 5 + ((1 << 33) if o >= 9000 else 0)


def _doc_tokens(o, rng, fill_w):
    """the pattern terms by ordinal (appended docs continue them), fillers of shifted Zipf weight"""
    all_tf = ALL_TF.get(o, 2 + (o // 16) % 4 if o % 16 == 5 else 1)
    toks = ["all"] * all_tf
    if o % 2 == 0:
        j = o // 2
        toks += ["half"] * (2 if j % 4 == 1 else 3 if j % 16 == 3 else 1)
    for name, where in (("flat", FLAT), ("gap", GAP), ("late", LATE), ("seam", SEAM), ("run", RUN)):
        if o in where:
            toks.append(name)
    for name, where in (("d1023", D1023), ("d1024", D1024), ("d1025", D1025)):
        if o in where:
            toks += [name] * (2 if o % 10 == 0 else 1)
    if o == N0 - 1:
        toks.append("one")
    toks += ["w%d" % x for x in rng.choices(range(N_FILLER), fill_w, k=rng.randint(1, 3))]
    return toks


def corpus_events():
    """-> (events, cut[5], ord_ids, info): events[:cut[k]] is the log of snapshot k; ord_ids the doc id of every
    ordinal a refreshed index ends with; info names what the snapshots remove and append."""
    import random
    rng = random.Random(20240611)
    # (1 / (i + 20): the heaviest filler stays well below df 1024, so the dense set is the designed one)
    fill_w = [1.0 / (i + 20) for i in range(N_FILLER)]
    events, ord_ids = [], []
    ghost_ids = []
    for o in range(N0):
        if o == 5000:
            # three docs whose only terms get adjacent ids, removed before the first load: empty rows side by side
            for g, name in enumerate(GHOSTS):
                ghost_ids.append(doc_id(o - 1) + 1 + g)
                events.append(("add", ghost_ids[-1], [name, name]))
        events.append(("add", doc_id(o), _doc_tokens(o, rng, fill_w)))
        ord_ids.append(doc_id(o))
    events += [("rm", g) for g in ghost_ids]
    cut = [len(events)]
    # 1: removals only
    events += [("rm", doc_id(o)) for o in RM1]
    cut.append(len(events))
    # 2: five appended docs, one new term
    nxt = (1 << 40) + 17

    def append(o, extra=()):
        nonlocal nxt
        events.append(("add", nxt, _doc_tokens(o, rng, fill_w) + list(extra)))
        ord_ids.append(nxt)
        nxt += 3 + (o % 4)
    for k in range(5):
        append(len(ord_ids), ("newterm",) if k in (1, 3) else ())
    cut.append(len(events))
    # 3: 40 removals (none of a d10xx doc: the dense set moves by d1023 alone) and 4100 appended docs, two of
    # them with d1023
    gone = set(RM1)
    keep = gone | D1023 | D1024 | D1025
    rm3 = [next(o for o in range(base, base + 20) if o not in keep) for base in range(200, N0, 400)][:40]
    assert len(rm3) == 40
    events += [("rm", doc_id(o)) for o in rm3]
    for k in range(N_APPEND3):
        append(len(ord_ids), ("d1023",) if k in (7, 2050) else ())
    cut.append(len(events))
    # 4: one appended doc whose tf of `all` is above every earlier one
    append(len(ord_ids), ["all"] * 300)
    cut.append(len(events))
    return events, cut, ord_ids, {"rm1": RM1, "rm3": tuple(rm3), "ghost_ids": tuple(ghost_ids)}


def n_ordinals(k):
    """ordinals of a refreshed index at snapshot k"""
    return N0 + (0, 0, 5, 5 + N_APPEND3, 6 + N_APPEND3)[k]


def fresh_ord_ids(events):
    """the ordinal table of an index loaded fresh: the live docs in file order"""
    _, docs, order = replay(events)
    return [d for d in order if d in docs]


# ---------------------------------------------------------------------------------------------------
# a doc shard: the shard view of a whole-index model
# ---------------------------------------------------------------------------------------------------

class ShardModel(Model):
    """One shard of a doc-sharded collection at the snapshot of `whole`, from the shard's ordinal table (its doc
    ids in load order, dead ones kept).

    collection-wide   the impact bits (the oracle's, restricted to the shard's docs: it scores with N, adl and df
                      of the whole collection), doc_count / token_count (the header scalars), the idf of a TF-IDF
                      cap (coll_live, coll_df), df_global
    local             everything structural: ordinals, df = list length, maximp (0 for a term without a local
                      posting, whatever its global df), the dense set and the bitmap rows (local df, local
                      n_docs), blkmap / bmrank, dense_col, the byte columns' bounds (local maximp), the tf list a
                      cap is picked from and the share n // outl_share it is picked with"""

    def __init__(self, whole, ord_ids):
        self.whole = whole
        self.terms, self.n_terms, self.oidx = whole.terms, whole.n_terms, None
        self.doc_count, self.token_count = whole.doc_count, whole.token_count
        self.ord_ids = np.asarray(ord_ids, dtype=np.uint64)
        self.ord_of = {int(d): o for o, d in enumerate(ord_ids)}
        assert len(self.ord_of) == len(ord_ids), "a doc id twice in one ordinal table"
        self.docs = {int(d): whole.docs[int(d)] for d in ord_ids if int(d) in whole.docs}
        self.live = np.array([int(d) in self.docs for d in ord_ids], dtype=bool)
        self.n_live = len(self.docs)
        mine = np.array(sorted(self.docs), dtype=np.uint64)
        if not hasattr(whole, "_canon_ids"):
            whole._canon_ids = {t: np.array([d for d, _ in r], dtype=np.uint64) for t, r in whole.canon.items()}
        self._mask = {t: np.isin(ids, mine) for t, ids in whole._canon_ids.items()}
        self.canon = {t: [whole.canon[t][i] for i in np.flatnonzero(k)] for t, k in self._mask.items()}
        self.df = {t: len(r) for t, r in self.canon.items()}
        self.ords = {t: np.array([self.ord_of[d] for d, _ in r], dtype=np.int64) for t, r in self.canon.items()}
        self.tfs = {t: whole.tfs[t][k] for t, k in self._mask.items()}
        for t, o in self.ords.items():
            assert (np.diff(o) > 0).all(), "doc ids must ascend with the shard's ordinals"
        self.coll_live, self.coll_df, self.coll_tokens = whole.n_live, whole.df, whole.coll_tokens

    def impacts(self, t, algo):
        return self.whole.impacts(t, algo)[self._mask[t]]

    def freeze(self):
        return self

    def df_global(self):
        return np.array([0] + [self.whole.df[t] for t in range(1, self.n_terms + 1)] + [0], dtype=np.uint32)


def even_slices(ids, n_shards):
    """N4 at open and at a full rebuild: shard s holds the live docs of rank [D s / S, D (s + 1) / S) by ascending id"""
    ids = sorted(ids)
    return [ids[len(ids) * s // n_shards:len(ids) * (s + 1) // n_shards] for s in range(n_shards)]


def shard_ord_tables(events, cut, n_shards, rebuilds=(), live=None):
    """-> per snapshot k (refreshed, fresh): the ordinal table of every shard of a collection opened at snapshot 0
    and refreshed to every later one, and of a collection opened fresh at k.  A refresh appends the new docs to the
    LAST shard and leaves a removed doc's ordinal (dead) on the shard that holds it; a snapshot in `rebuilds` is
    taken by a full rebuild, which slices again.  (live[k]: the live doc ids of snapshot k, if the caller has them.)"""
    out, tabs = [], None
    for k in range(len(cut)):
        fresh = even_slices(live[k] if live else replay(events[:cut[k]])[1], n_shards)
        if k == 0 or k in rebuilds:
            tabs = [list(x) for x in fresh]
        else:
            tabs = [list(x) for x in tabs]
            tabs[-1] += [e[1] for e in events[cut[k - 1]:cut[k]] if e[0] == "add"]
        out.append((tabs, fresh))
    return out


def table_max_tf(events, ord_ids):
    """max_tf of an index that holds (or held) these docs: a refresh never lowers it"""
    mine = set(int(d) for d in ord_ids)
    return max(max(e[2].count(t) for t in set(e[2])) for e in events if e[0] == "add" and e[1] in mine)


# ---------------------------------------------------------------------------------------------------
# the checker of one image (whole index or shard) and the image a model stands for
# ---------------------------------------------------------------------------------------------------

ALGO_NAME = {TF_IDF: "TF-IDF", BM25: "BM25"}
SWITCHES = (0.05, 8, 1 << 30)       # scanm_dens, outl_share, bm_share of the image tests


def flat_rows(img):
    """-> (row of every posting, its ordinal, its tf)"""
    off = img["post_off"].astype(np.int64)
    dt = img["post_dt"]
    row = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return off, row, (dt >> np.uint64(32)).astype(np.int64), (dt & np.uint64(0xffffffff)).astype(np.int64)


def check_image(img, m, max_tf, ctx, algos=ALGOS):
    """Every array of one image against the model m (whose ordinal table is this index's).  The statistics of the
    ranking functions are the model's collection-wide ones (m.coll_live, m.coll_df, m.coll_tokens: on a whole
    index its own); `algos`: the ranking functions that are materialised -- the parts of the others must be absent."""
    sc = img["scalars"]
    n_docs, T_ = len(m.ord_ids), m.n_terms
    P = sum(m.df.values())
    # ---- scalars
    assert sc["n_docs"] == n_docs and sc["n_terms"] == T_ and sc["n_post"] == P, (ctx, sc)
    assert sc["hdr_doc_count"] == m.coll_live == m.doc_count, (ctx, sc)
    assert sc["hdr_token_count"] == m.coll_tokens == m.token_count, (ctx, sc)
    assert sc["max_tf"] == max_tf, (ctx, sc["max_tf"], max_tf)
    assert sc["bm_words"] == (n_docs + 4095) // 4096, (ctx, sc)
    assert sc["dense_q8_stride"] == ((n_docs + 16383) & ~16383) + 16384, (ctx, sc)
    assert sc["cap_post"] >= P and sc["algo_on"] == sum(1 << a for a in algos), (ctx, sc)
    assert (sc["scanm_dens"], sc["outl_share"], sc["bm_share"]) == SWITCHES, (ctx, sc)
    # ---- the collection-wide df of a doc shard
    want_g = m.df_global()
    if want_g is None:
        assert img.get("df_global") is None, (ctx, "df_global", "on an index that is no shard")
    else:
        got_g = img["df_global"]
        assert got_g is not None and len(got_g) == T_ + 2, (ctx, "df_global", "absent or of the wrong length")
        bad = np.flatnonzero(got_g != want_g)
        assert not len(bad), (ctx, "df_global", bad[:8], got_g[bad[:8]], want_g[bad[:8]])
    # ---- docs and CSR
    assert len(img["doc_ids"]) == n_docs == len(img["doc_len"]), ctx
    assert np.array_equal(img["doc_ids"][m.live], m.ord_ids[m.live]), ctx
    want_len = np.array([m.docs[int(d)][0] if lv else 0 for d, lv in zip(m.ord_ids, m.live)], dtype=np.uint32)
    assert np.array_equal(img["doc_len"][m.live], want_len[m.live]), ctx
    off, row, doc, tf = flat_rows(img)
    assert len(off) == T_ + 2 and off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == P == len(img["post_dt"]), ctx
    same_row = row[1:] == row[:-1]
    assert (np.diff(doc)[same_row] > 0).all(), (ctx, "ordinals of a row must ascend strictly")
    assert (doc < n_docs).all() and m.live[doc].all(), (ctx, "a posting of a dead or unknown ordinal")
    want_off = np.concatenate([[0, 0], np.cumsum([m.df[t] for t in range(1, T_ + 1)])])
    assert np.array_equal(off, want_off), (ctx, np.flatnonzero(off != want_off)[:8])
    want_doc = np.concatenate([m.ords[t] for t in range(1, T_ + 1)])
    want_tf = np.concatenate([m.tfs[t] for t in range(1, T_ + 1)])
    bad = np.flatnonzero((doc != want_doc) | (tf != want_tf))
    assert not len(bad), (ctx, "canonical postings", bad[:8], row[bad[:8]])
    # ---- impacts and per-term maxima, every materialised ranking function
    for a in ALGOS:
        post, mx = img[("post", a)], img[("maximp", a)]
        if a not in algos:
            assert post.size == 0 and mx.size == 0 and img[("dense_col", a)].size == 0, (ctx, ALGO_NAME[a], "not materialised")
            continue
        assert len(post) == P, (ctx, a)
        assert np.array_equal(post["doc"].astype(np.int64), doc), (ctx, a)
        want = np.concatenate([m.impacts(t, a) for t in range(1, T_ + 1)])
        bad = np.flatnonzero(post["imp"] != want)
        assert not len(bad), (ctx, ALGO_NAME[a], "impact bits", bad[:8], row[bad[:8]], post["imp"][bad[:4]], want[bad[:4]])
        want_mx = np.array([0] + [m.maximp(t, a) for t in range(1, T_ + 1)] + [0], dtype=np.uint32)
        bad = np.flatnonzero(mx != want_mx)
        assert len(mx) == T_ + 2 and not len(bad), (ctx, ALGO_NAME[a], "maximp", bad[:8], mx[bad[:8]], want_mx[bad[:8]])
    # ---- block-presence bitmaps and rank directories
    words = sc["bm_words"]
    bm_terms = img["bm_terms"].tolist()
    assert bm_terms == m.bm_terms(n_docs, sc["bm_share"]), ctx
    assert bm_terms == [t for t in range(1, T_ + 1) if m.df[t] > 0], ctx           # (with this share: every list)
    blk = img["blkmap"].reshape(len(bm_terms), words)
    rnk = img["bmrank"].reshape(len(bm_terms), words + 1)
    for r, t in enumerate(bm_terms):
        assert np.array_equal(blk[r], m.blkmap(t, words)), (ctx, "blkmap", m.terms[t - 1], blk[r], m.blkmap(t, words))
        assert np.array_equal(rnk[r], m.bmrank(t, words)), (ctx, "bmrank", m.terms[t - 1], rnk[r], m.bmrank(t, words))
    # ---- dense columns
    dense = img["dense_terms"].tolist()
    assert dense == m.dense_terms(n_docs, sc["scanm_dens"]), (ctx, "dense_terms", dense)
    nc = len(dense)
    for a in algos:
        col = img[("dense_col", a)].reshape(nc, n_docs)
        for c, t in enumerate(dense):
            bad = np.flatnonzero(col[c] != m.dense_col(t, a, n_docs))
            assert not len(bad), (ctx, ALGO_NAME[a], "dense_col", m.terms[t - 1], bad[:8])
    # ---- byte columns (BM25): 0 where the doc lacks the term and in the padding; for a posting
    # max(L, 1) <= q8 <= min(255, L + 1), L = ceil(255 imp / max) exactly
    q8 = img["dense_q8"]
    assert q8.shape == (nc, sc["dense_q8_stride"]), (ctx, q8.shape)
    for c, t in enumerate(dense):
        lo, hi = q8_bounds(m.impacts(t, BM25), m.maximp(t, BM25))
        got = q8[c][m.ords[t]].astype(np.int64)
        bad = np.flatnonzero((got < lo) | (got > hi))
        assert not len(bad), (ctx, "dense_q8", m.terms[t - 1], bad[:8], got[bad[:8]], lo[bad[:8]], hi[bad[:8]])
        rest = q8[c].copy()
        rest[m.ords[t]] = 0
        assert not rest.any(), (ctx, "dense_q8 cells without a posting", m.terms[t - 1], np.flatnonzero(rest)[:8])
    # ---- TF-IDF caps and outlier lists
    if TF_IDF not in algos:
        for key in ("outl_off", "outl_cap", "outl_max", "outl_post"):
            assert img[key].size == 0, (ctx, key, "TF-IDF is not materialised")
        return {"dense": dense, "bm_rows": len(bm_terms)}
    o_off, o_post = img["outl_off"].astype(np.int64), img["outl_post"]
    assert len(o_off) == nc + 1 and len(img["outl_cap"]) == nc == len(img["outl_max"]), ctx
    assert o_off[0] == sc["cap_post"] and (np.diff(o_off) >= 0).all() and len(o_post) == o_off[-1] - o_off[0], ctx
    for c, t in enumerate(dense):
        cap, ords, xb, cap_bits, max_bits = m.outliers(t, sc["outl_share"])
        lst = o_post[o_off[c] - o_off[0]:o_off[c + 1] - o_off[0]]
        who = (ctx, "outliers", m.terms[t - 1], cap)
        assert np.array_equal(lst["doc"].astype(np.int64), ords), who
        assert np.array_equal(lst["imp"], xb), (who, lst["imp"][:4], xb[:4])
        assert int(img["outl_cap"][c]) == cap_bits and int(img["outl_max"][c]) == max_bits, \
            (who, int(img["outl_cap"][c]), cap_bits, int(img["outl_max"][c]), max_bits)
    return {"dense": dense, "bm_rows": len(bm_terms)}


def canonical(img):
    """per posting (term, doc id, tf, impact bits under both functions), and the per-term maxima: what a
    refreshed and a freshly loaded index must agree on (ordinals and the dense set may differ)"""
    _, row, doc, tf = flat_rows(img)
    return (row, img["doc_ids"][doc], tf, img[("post", TF_IDF)]["imp"], img[("post", BM25)]["imp"],
            img[("maximp", TF_IDF)], img[("maximp", BM25)])


POST_T = np.dtype([("doc", "<u4"), ("imp", "<u4")])


def image_of(m, max_tf):
    """The image the model stands for, in the form Index.device_image() returns (both functions materialised, the
    image tests' switches; every byte-column cell at its lower bound): what check_image must accept whole, and
    what the CPU tier perturbs one value at a time."""
    n_docs, T_ = len(m.ord_ids), m.n_terms
    rows = range(1, T_ + 1)
    P = sum(m.df.values())
    words, stride = (n_docs + 4095) // 4096, ((n_docs + 16383) & ~16383) + 16384
    cap_post = P + P // 16 + 4096
    img = {"scalars": {"n_docs": n_docs, "n_post": P, "n_terms": T_, "hdr_doc_count": m.doc_count,
                       "hdr_token_count": m.token_count, "max_tf": max_tf, "bm_words": words, "dense_q8_stride": stride,
                       "cap_post": cap_post, "scanm_dens": SWITCHES[0], "outl_share": SWITCHES[1], "bm_share": SWITCHES[2],
                       "algo_on": 3, "switches": 7}}
    img["doc_ids"] = m.ord_ids.copy()
    img["doc_len"] = np.array([m.docs[int(d)][0] if lv else 0 for d, lv in zip(m.ord_ids, m.live)], dtype=np.uint32)
    img["post_off"] = np.concatenate([[0, 0], np.cumsum([m.df[t] for t in rows])]).astype(np.uint64)
    ords = np.concatenate([m.ords[t] for t in rows]).astype(np.uint64)
    img["post_dt"] = (ords << np.uint64(32)) | np.concatenate([m.tfs[t] for t in rows]).astype(np.uint64)
    for a in ALGOS:
        post = np.zeros(P, dtype=POST_T)
        post["doc"], post["imp"] = ords, np.concatenate([m.impacts(t, a) for t in rows])
        img[("post", a)] = post
        img[("maximp", a)] = np.array([0] + [m.maximp(t, a) for t in rows] + [0], dtype=np.uint32)
    bm = m.bm_terms(n_docs, SWITCHES[2])
    img["bm_terms"] = np.array(bm, dtype=np.uint32)
    img["blkmap"] = np.concatenate([m.blkmap(t, words) for t in bm]) if bm else np.zeros(0, np.uint64)
    img["bmrank"] = np.concatenate([m.bmrank(t, words) for t in bm]) if bm else np.zeros(0, np.uint32)
    dense = m.dense_terms(n_docs, SWITCHES[0])
    img["dense_terms"] = np.array(dense, dtype=np.uint32)
    for a in ALGOS:
        img[("dense_col", a)] = np.concatenate([m.dense_col(t, a, n_docs) for t in dense]) if dense else np.zeros(0, np.uint32)
    q8 = np.zeros((len(dense), stride), dtype=np.uint8)
    lists, off = [], [cap_post]
    caps, maxes = [], []
    for c, t in enumerate(dense):
        q8[c][m.ords[t]] = q8_bounds(m.impacts(t, BM25), m.maximp(t, BM25))[0]
        _, o, xb, cap_bits, max_bits = m.outliers(t, SWITCHES[1])
        lst = np.zeros(len(o), dtype=POST_T)
        lst["doc"], lst["imp"] = o, xb
        lists.append(lst)
        off.append(off[-1] + len(o))
        caps.append(cap_bits)
        maxes.append(max_bits)
    img["dense_q8"] = q8
    img["outl_off"] = np.array(off, dtype=np.uint64)
    img["outl_post"] = np.concatenate(lists) if lists else np.zeros(0, dtype=POST_T)
    img["outl_cap"], img["outl_max"] = np.array(caps, dtype=np.uint32), np.array(maxes, dtype=np.uint32)
    img["df_global"] = m.df_global()
    return img


# ---------------------------------------------------------------------------------------------------
# the corpus of the doc-shard image tests: one log per shard count, six snapshots, the edges inside EVERY shard
# ---------------------------------------------------------------------------------------------------
#
# A collection of S x SH_M docs: at open shard s holds the ranks [SH_M s, SH_M (s + 1)), so a doc's tokens are a
# function of its shard and LOCAL ordinal.  The schedule of ids (what every snapshot removes and appends) is laid
# down first; from it follows where every doc lies after the full rebuild of snapshot 5 slices again, and a second
# set of pattern terms (r...) is placed by THAT shard and local ordinal: the seams and the list lengths around 1024
# are inside every shard before and after the slices move.

SH_M = 2 * 4096 + 7                     # docs per shard at snapshot 0: two bitmap words and 7 docs of a third
SH_ALL_TF = {100: 40, 3000: 62, 5000: 63, 6000: 64, 8000: 200}
SH_E = {"ea": (3, 7), "eb": (5, 7), "ec": (1, 6)}       # first local ordinal, stride; 1023 / 1024 / 1025 docs, rotated by shard
SH_ED = (4, 5, 1022)                    # `ed`: 1022 docs in every shard
SH_FLAT = range(1500, 7500, 3)          # 2000 docs, tf 1: dense, no cap
SH_EARLY = frozenset(10 + 7 * i for i in range(20))                     # bitmap word 0 only
SH_LATE = frozenset(4096 + 50 + 100 * i for i in range(30))             # bitmap word 1 only
SH_SEAM = (63, 64, 4095, 4096, 8191, 8192)
SH_ONLY = frozenset(20 + 400 * i for i in range(15))                    # `only0` / `onlylast`: one shard holds them all
SH_RM1 = (0, SH_M - 1, 4100, 47)        # snapshot 1, in EVERY shard (moved to the next ordinal without an e-term)
SH_N_APPEND2, SH_N_APPEND3, SH_N_RM3 = 5, 2100, 12
SH_SNAPSHOTS = 6


def _e_len(name, s):
    return (1023, 1024, 1025)[(s + ("ea", "eb", "ec").index(name)) % 3]


def _in_stride(o, first, stride, n):
    return o >= first and (o - first) % stride == 0 and (o - first) // stride < n


def _has_e(o):
    return any(_in_stride(o, f, st, 1025) for f, st in SH_E.values()) or _in_stride(o, *SH_ED)


def _free_from(o):
    """the next local ordinal at or above o whose doc carries no e-term (their list lengths are designed)"""
    while _has_e(o):
        o += 1
    return o


def _placed_tokens(prefix, s, o):
    """the pattern terms a doc of shard s at local ordinal o carries (prefix "": by the slices of snapshot 0,
    "r": by those of snapshot 5)"""
    toks = []
    for name, (first, stride) in SH_E.items():
        if _in_stride(o, first, stride, _e_len(name, s)):
            toks += [prefix + name] * (2 if o % 10 == 0 else 1)
    if _in_stride(o, *SH_ED):
        toks.append(prefix + "ed")
    for name, where in (("early", SH_EARLY), ("late", SH_LATE), ("seam", SH_SEAM)):
        if o in where:
            toks.append(prefix + name)
    return toks


def _shard_doc_tokens(s, o, n_shards, rng, fill_w):
    all_tf = SH_ALL_TF.get(o, 2 + (o // 16) % 4 if o % 16 == 5 else 1)
    toks = ["all"] * all_tf
    if o % 2 == 0:
        j = o // 2
        toks += ["half"] * (2 if j % 4 == 1 else 3 if j % 16 == 3 else 1)
    if o in SH_FLAT:
        toks.append("flat")
    if o in SH_ONLY and s == 0:
        toks.append("only0")
    if o in SH_ONLY and s == n_shards - 1:
        toks.append("onlylast")
    toks += _placed_tokens("", s, o)
    toks += ["w%d" % x for x in rng.choices(range(N_FILLER), fill_w, k=rng.randint(1, 3))]
    return toks


def shard_corpus_events(n_shards):
    """-> (events, cut[6], info): events[:cut[k]] is the log of snapshot k of a collection of n_shards shards.
    0 fresh; 1 removals only, in every shard; 2 appends only (they go to the last shard; the other shards' share
    is empty) that move N, the integer adl and the term count; 3 removals in every shard and more appended docs
    than the last shard's d_post and spare CSR buffer hold, a new term, and the last shard's 1023-list grows to
    1025 (its dense set moves); 4 one doc with a new largest tf; 5 an id below the highest: a full rebuild."""
    import random
    S = n_shards
    rng = random.Random(20250302 + S)
    fill_w = [1.0 / (i + 20) for i in range(N_FILLER)]
    # ---- the schedule: ids alone
    first = [(s, o, doc_id(SH_M * s + o)) for s in range(S) for o in range(SH_M)]
    id_at = {(s, o): d for s, o, d in first}
    ghost_ids = [doc_id(5000 - 1) + 1 + g for g in range(len(GHOSTS))]
    rm1 = [id_at[(s, _free_from(o) if o < SH_M - 1 else o)] for s in range(S) for o in SH_RM1]
    rm3 = [id_at[(s, _free_from(300 + 650 * i))] for s in range(S) for i in range(SH_N_RM3)]
    assert len(set(rm1 + rm3)) == len(rm1) + len(rm3) and not _has_e(SH_M - 1)
    nxt, appended = (1 << 40) + 17, []          # (id, local ordinal on the last shard)
    for i in range(SH_N_APPEND2 + SH_N_APPEND3 + 1):
        appended.append((nxt, SH_M + i))
        nxt += 3 + (i % 4)
    odd_id = doc_id(SH_M // 2) + 7              # snapshot 5: an unused id inside shard 0's range
    final = sorted(({d for _, _, d in first} | {d for d, _ in appended} | {odd_id}) - set(rm1) - set(rm3))
    place5 = {d: (s, o) for s, ids in enumerate(even_slices(final, S)) for o, d in enumerate(ids)}
    r_tokens = lambda d: _placed_tokens("r", *place5[d]) if d in place5 else []
    # ---- the log
    events = []
    for s, o, d in first:
        if (s, o) == (0, 5000):
            events += [("add", g, [name, name]) for g, name in zip(ghost_ids, GHOSTS)]
        events.append(("add", d, _shard_doc_tokens(s, o, S, rng, fill_w) + r_tokens(d)))
    events += [("rm", g) for g in ghost_ids]
    cut = [len(events)]
    events += [("rm", d) for d in rm1]
    cut.append(len(events))
    # 2: five docs; ballast on them lifts the integer average doc length (the adl of BM25) by one
    tokens = sum(len(e[2]) for e in events if e[0] == "add") - 2 * len(GHOSTS)
    gone = set(rm1)
    tokens -= sum(len(e[2]) for e in events if e[0] == "add" and e[1] in gone)
    n_live = S * SH_M - len(rm1)
    last = S - 1
    docs2 = [(d, _shard_doc_tokens(last, o, S, rng, fill_w) + r_tokens(d) + (["newterm"] if i in (1, 3) else []))
             for i, (d, o) in enumerate(appended[:SH_N_APPEND2])]
    need = (tokens // n_live + 1) * (n_live + SH_N_APPEND2) - tokens - sum(len(t) for _, t in docs2) + 64
    per_doc = -(-need // SH_N_APPEND2)
    assert 0 < per_doc <= 60 * 100, per_doc
    for i, (d, toks) in enumerate(docs2):
        ballast = []
        for j in range(60):
            ballast += ["w%d" % ((7 * i + j) % N_FILLER)] * min(100, max(0, per_doc - 100 * j))
        events.append(("add", d, toks + ballast))
    cut.append(len(events))
    # 3: removals in every shard, 2100 appended docs: two carry the last shard's 1023-list, one `ed`, two a new term
    grow = next(name for name in SH_E if _e_len(name, last) == 1023)
    events += [("rm", d) for d in rm3]
    for i, (d, o) in enumerate(appended[SH_N_APPEND2:SH_N_APPEND2 + SH_N_APPEND3]):
        extra = [grow] if i in (7, 1050) else ["ed"] if i == 9 else ["newterm3", "newterm3"] if i in (11, 2000) else []
        events.append(("add", d, _shard_doc_tokens(last, o, S, rng, fill_w) + r_tokens(d) + extra))
    cut.append(len(events))
    # 4: one doc whose tf of `all` is above every earlier tf
    d, o = appended[-1]
    events.append(("add", d, _shard_doc_tokens(last, o, S, rng, fill_w) + r_tokens(d) + ["all"] * 300))
    cut.append(len(events))
    # 5: an id below the highest one: no refresh can append it, every shard rebuilds its slice
    events.append(("add", odd_id, ["all", "half", "oddterm"] + r_tokens(odd_id)))
    cut.append(len(events))
    return events, cut, {"rm1": rm1, "rm3": rm3, "ghost_ids": ghost_ids, "odd_id": odd_id, "grow": grow,
                         "place5": place5}


class ShardTruth:
    """Everything the doc-shard image tests compare with, for one shard count: every snapshot written to files of
    its own (never rewritten: the oracle maps them), its whole-index model with the oracle asked at once, the
    shard views of a collection refreshed through the snapshots and of one opened fresh, and the oracle's answer
    to `all OR half` under both functions."""
    QUERY = "all OR half"

    def __init__(self, base, n_shards):
        import nxsfmt
        import oracle_lib as O
        self.S = n_shards
        self.events, self.cut, self.info = shard_corpus_events(n_shards)
        played = [replay(self.events[:c]) for c in self.cut]
        self.tables = shard_ord_tables(self.events, self.cut, n_shards, rebuilds=(5,), live=[p[1] for p in played])
        self.whole, self.shards, self.fresh, self.want, self.images = [], [], [], [], []
        for k in range(SH_SNAPSHOTS):
            ev = self.events[:self.cut[k]]
            timg, dimg, _ = nxsfmt.build_images_log(ev)
            self.images.append((timg, dimg))
            t, d = str(base / ("t%d_%d" % (n_shards, k))), str(base / ("d%d_%d" % (n_shards, k)))
            open(t, "wb").write(timg)
            open(d, "wb").write(dimg)
            oidx = O.Index(t, d)
            whole = Model(ev, oidx, sorted(played[k][1]), replayed=played[k]).freeze()
            self.want.append([oidx.search(self.QUERY, limit=10, algo=a) for a in (BM25, TF_IDF)])
            oidx.close()
            self.whole.append(whole)
            refreshed, fresh = self.tables[k]
            self.shards.append([ShardModel(whole, tab) for tab in refreshed])
            self.fresh.append([ShardModel(whole, tab) for tab in fresh])

    def max_tf(self, k, s, fresh=False):
        return table_max_tf(self.events[:self.cut[k]], self.tables[k][1 if fresh else 0][s])
