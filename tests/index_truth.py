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

    def __init__(self, events, oidx, ord_ids):
        self.terms, self.docs, _ = replay(events)
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
        cap_imp = tfidf_cap_imp(cap, self.n_live, self.df[t])
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
