"""Host model of the term-side device state, and the corpus the term-image tests run on.

Plain Python and numpy; no code of the library.  A snapshot is the dictionary (term id -> bytes, in file order),
the on-disk total of every term and its live df.  The totals are read from the nxsterms file by read_terms (the
oracle has no accessor for them; it gives the df and confirms the bytes) when the snapshot is made: the next
snapshot rewrites the files in place.

From those the model states what every array of Index.term_image() must hold:

  the tree         terms inserted in term-id order; at a node the distance to its term (a row DP over bytes, written
                   here) picks the child slot, distances above 63 share slot 63, distance 0 is a duplicate
  bk / bk_bytes    the nodes in BFS order, the children of a node contiguous in ascending slot: bitmap of the
                   child slots, first_child (for a leaf: where its children would begin), term_id, str_off /
                   str_len into the byte pool (the terms in node order), flag bit 0 = total > 0, inl = the first
                   8 bytes, zero padded; bk_depth = the number of levels
  bk_parent/_slot  per node; 0xffffffff and 0 for the root
  fz_*             the nodes with flag bit 0 set and at most 66 bytes that do not hang below a slot-63 child, by
                   length and then by node (a stable counting sort); signature = OR of 1 << (byte & 31); the
                   length; fz_len_start[l] = the first candidate of length l, l = 0 .. 67
  sg_*             the nodes with live df > 0 and at most 66 bytes, wherever they hang and whatever the flag says;
                   the same order and signatures
  px_*             the nodes with live df > 0, any length, strictly ascending by their unsigned bytes (a proper
                   prefix before its extensions); key = (~df & 0xffffffff) << 32 | term id

check_term_image compares one image with a model, part by part; image_of makes the image a model stands for.
corpus() is the event log of tests/test_term_image.py with every designed edge placed by construction, and
preconditions() asserts, from a model alone, that the edges are there at the snapshot that needs them.
"""
import random
import struct

import numpy as np

FZ_MAXLEN = 66
NOPARENT = 0xffffffff
BK_DTYPE = np.dtype([("bitmap", "<u8"), ("first_child", "<u4"), ("term_id", "<u4"), ("str_off", "<u4"),
                     ("str_len", "<u2"), ("flags", "<u2"), ("inl", "u1", (8,))])
PARTS = ("bk", "fz", "sg", "px")

_lev = {}


def levdist(a, b):
    """Levenshtein distance of two byte strings: one DP row, unit costs"""
    if a == b:
        return 0
    key = (a, b) if a <= b else (b, a)
    d = _lev.get(key)
    if d is None:
        s, t = key if len(key[0]) >= len(key[1]) else (key[1], key[0])       # the row runs over the shorter one
        row = list(range(len(t) + 1))
        for i, cs in enumerate(s, 1):
            diag, row[0] = row[0], i
            for j, ct in enumerate(t, 1):
                cur = row[j]
                v = diag if cs == ct else diag + 1
                if cur + 1 < v:
                    v = cur + 1
                if row[j - 1] + 1 < v:
                    v = row[j - 1] + 1
                row[j] = v
                diag = cur
        d = _lev[key] = row[-1]
    return d


def read_terms(path_or_bytes):
    """the nxsterms file -> ([term bytes], [total]) in term-id order (u16 length, the bytes, a NUL, padding to 8,
    a u64 total; all big-endian, behind a 16-byte header that holds the data length)"""
    img = path_or_bytes if isinstance(path_or_bytes, bytes) else open(path_or_bytes, "rb").read()
    assert img[:5] == b"NXS_T"
    data_len, = struct.unpack(">I", img[8:12])
    terms, totals, off = [], [], 16
    while off < 16 + data_len:
        ln, = struct.unpack(">H", img[off:off + 2])
        blk = ((2 + ln + 1 + 7) & ~7) + 8
        terms.append(img[off + 2:off + 2 + ln])
        totals.append(struct.unpack(">Q", img[off + blk - 8:off + blk])[0])
        off += blk
    return terms, totals


def set_totals(timg, totals):
    """the nxsterms image with the on-disk total of some terms replaced: {term bytes: total}"""
    img, off = bytearray(timg), 16
    data_len, = struct.unpack(">I", img[8:12])
    left = dict(totals)
    while off < 16 + data_len:
        ln, = struct.unpack(">H", img[off:off + 2])
        blk = ((2 + ln + 1 + 7) & ~7) + 8
        t = bytes(img[off + 2:off + 2 + ln])
        if t in left:
            img[off + blk - 8:off + blk] = struct.pack(">Q", left.pop(t))
        off += blk
    assert not left, left
    return bytes(img)


def signature(t):
    s = 0
    for c in t:
        s |= 1 << (c & 31)
    return s


class TermModel:
    """terms, totals, dfs: lists in term-id order (index i is term id i + 1).  Everything is computed here, once."""

    def __init__(self, terms, totals, dfs):
        assert len(terms) == len(totals) == len(dfs) and len(set(terms)) == len(terms)
        self.terms, self.totals, self.dfs = list(terms), list(totals), list(dfs)
        # ---- the tree, in insertion order: [term index, {slot: build index}]
        build = []
        for ti, t in enumerate(self.terms):
            if not build:
                build.append((ti, {}))
                continue
            cur = 0
            while True:
                d = levdist(t, self.terms[build[cur][0]])
                if d == 0:
                    break
                d = min(d, 63)
                nxt = build[cur][1].get(d)
                if nxt is None:
                    build[cur][1][d] = len(build)
                    build.append((ti, {}))
                    break
                cur = nxt
        # ---- BFS numbering
        n = len(build)
        order, level = ([0], [0]) if n else ([], [])
        bitmap, first_child = [0] * n, [0] * n
        parent, slot = [NOPARENT] * n, [0] * n
        head = 0
        while head < len(order):
            kids = build[order[head]][1]
            first_child[head] = len(order)
            for sl in sorted(kids):
                bitmap[head] |= 1 << sl
                parent[len(order)], slot[len(order)] = head, sl
                level.append(level[head] + 1)
                order.append(kids[sl])
            head += 1
        assert len(order) == n
        self.n = n
        self.depth = level[-1] + 1 if n else 0
        self.node_term = [build[b][0] for b in order]                  # node -> term index
        bk = np.zeros(n, dtype=BK_DTYPE)
        pool = bytearray()
        for i, ti in enumerate(self.node_term):
            t = self.terms[ti]
            bk[i] = (bitmap[i], first_child[i], ti + 1, len(pool), len(t), 1 if self.totals[ti] > 0 else 0,
                     list(t[:8].ljust(8, b"\0")))
            pool += t
        self.bk, self.pool = bk, np.frombuffer(bytes(pool), dtype=np.uint8)
        self.parent = np.array(parent, dtype=np.uint32)
        self.slot = np.array(slot, dtype=np.uint8)
        # ---- below a slot-63 child (a parent precedes its children)
        cut = [False] * n
        for i in range(1, n):
            cut[i] = cut[parent[i]] or slot[i] >= 63
        self.cut = cut
        nt = lambda i: self.terms[self.node_term[i]]
        df = lambda i: self.dfs[self.node_term[i]]
        by_len = lambda nodes: sorted(nodes, key=lambda i: (len(nt(i)), i))
        self.fz = by_len(i for i in range(n) if bk["flags"][i] & 1 and len(nt(i)) <= FZ_MAXLEN and not cut[i])
        self.sg = by_len(i for i in range(n) if df(i) > 0 and len(nt(i)) <= FZ_MAXLEN)
        self.px = sorted((i for i in range(n) if df(i) > 0), key=nt)
        self.fz_len_start = np.array([sum(1 for i in self.fz if len(nt(i)) < l) for l in range(FZ_MAXLEN + 2)],
                                     dtype=np.uint32)
        self.px_key = np.array([((~df(i)) & 0xffffffff) << 32 | (self.node_term[i] + 1) for i in self.px], dtype=np.uint64)

    def term_of(self, node):
        return self.terms[self.node_term[node]]

    def node_of(self, term):
        return self.node_term.index(self.terms.index(term))

    def cand_arrays(self, nodes):
        """-> (node u32, signature u32, length u8) of a candidate list"""
        return (np.array(nodes, dtype=np.uint32), np.array([signature(self.term_of(i)) for i in nodes], dtype=np.uint32),
                np.array([len(self.term_of(i)) for i in nodes], dtype=np.uint8))


def image_of(m, sg_gen=1, px_gen=1, px_builds=1):
    """the image (Index.term_image) the model stands for, every lazily built part built for the current generation"""
    fz, sg = m.cand_arrays(m.fz), m.cand_arrays(m.sg)
    sc = {"n_bk": m.n, "bk_depth": m.depth, "bk_bytes_len": len(m.pool), "n_fz": len(m.fz),
          "sg_gen": sg_gen, "sg_built": 1, "sg_built_gen": sg_gen, "sg_n_c": len(m.sg),
          "px_gen": px_gen, "px_built": 1, "px_built_gen": px_gen, "px_n_e": len(m.px), "px_builds": px_builds}
    e4, e1 = np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    return {"scalars": sc, "bk": m.bk.copy(), "bk_bytes": m.pool.copy(),
            "bk_parent": m.parent.copy() if m.n else e4, "bk_slot": m.slot.copy() if m.n else e1,
            "fz_node": fz[0], "fz_sig": fz[1], "fz_len": fz[2], "fz_len_start": m.fz_len_start.copy() if m.n else e4,
            "sg_node": sg[0], "sg_sig": sg[1], "sg_len": sg[2],
            "px_node": np.array(m.px, dtype=np.uint32), "px_key": m.px_key.copy()}


def _same(ctx, part, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (ctx, part, "length", got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (ctx, part, "index", int(bad[0]), "got", got[bad[0]].item(), "want", want[bad[0]].item(),
                          "mismatches", len(bad))


def _cands(ctx, name, img, m, want_nodes):
    """one candidate list (fz / sg): the nodes, then signature and length of every entry"""
    node, sig, ln = img[name + "_node"], img[name + "_sig"], img[name + "_len"]
    w_node, w_sig, w_len = m.cand_arrays(want_nodes)
    assert len(node) == len(sig) == len(ln), (ctx, name, "lengths of the three arrays", len(node), len(sig), len(ln))
    _same(ctx, name + "_node", node, w_node)
    missing = np.flatnonzero(w_sig & ~sig)
    assert not len(missing), (ctx, name + "_sig", "index", int(missing[0]), "bits missing", hex(int(w_sig[missing[0]] & ~sig[missing[0]])),
                              "got", hex(int(sig[missing[0]])), "want", hex(int(w_sig[missing[0]])))
    extra = np.flatnonzero(sig & ~w_sig)
    assert not len(extra), (ctx, name + "_sig", "index", int(extra[0]), "bits too many", hex(int(sig[extra[0]] & ~w_sig[extra[0]])),
                            "got", hex(int(sig[extra[0]])), "want", hex(int(w_sig[extra[0]])))
    _same(ctx, name + "_len", ln, w_len)


def check_term_image(img, m, ctx, parts=PARTS):
    """One image against the model.  parts: "bk" the BK image and its side arrays, "fz" the match-first candidates,
    "sg" suggest's, "px" the order -- the lazily built ones are compared once the call that builds them has run,
    and must then be built for the index's current generation."""
    sc = img["scalars"]
    if "bk" in parts:
        assert sc["n_bk"] == m.n == len(img["bk"]), (ctx, "scalars", "n_bk", sc["n_bk"], m.n, len(img["bk"]))
        assert sc["bk_depth"] == m.depth, (ctx, "scalars", "bk_depth", sc["bk_depth"], m.depth)
        assert sc["bk_bytes_len"] == len(m.pool), (ctx, "scalars", "bk_bytes_len", sc["bk_bytes_len"], len(m.pool))
        for f in ("bitmap", "first_child", "term_id", "str_off", "str_len", "flags"):
            _same(ctx, "bk." + f, img["bk"][f], m.bk[f])
        _same(ctx, "bk.inl", img["bk"]["inl"].copy().view("<u8").ravel(), m.bk["inl"].copy().view("<u8").ravel())
        _same(ctx, "bk_bytes", img["bk_bytes"], m.pool)
        _same(ctx, "bk_parent", img["bk_parent"], m.parent if m.n else m.parent[:0])
        _same(ctx, "bk_slot", img["bk_slot"], m.slot if m.n else m.slot[:0])
    if "fz" in parts:
        assert sc["n_fz"] == len(m.fz), (ctx, "scalars", "n_fz", sc["n_fz"], len(m.fz))
        for i, nd in enumerate(img["fz_node"].tolist()):
            assert nd < m.n and not m.cut[nd], (ctx, "fz_node", "index", i, "node", nd, "hangs below a slot-63 child")
        _cands(ctx, "fz", img, m, m.fz)
        _same(ctx, "fz_len_start", img["fz_len_start"], m.fz_len_start if m.n else m.fz_len_start[:0])
    if "sg" in parts:
        assert sc["sg_built"] == 1 and sc["sg_built_gen"] == sc["sg_gen"], (ctx, "scalars", "suggest's candidates are stale", sc)
        assert sc["sg_n_c"] == len(m.sg), (ctx, "scalars", "sg_n_c", sc["sg_n_c"], len(m.sg))
        _cands(ctx, "sg", img, m, m.sg)
    if "px" in parts:
        assert sc["px_built"] == 1 and sc["px_built_gen"] == sc["px_gen"], (ctx, "scalars", "the order is stale", sc)
        assert sc["px_n_e"] == len(m.px), (ctx, "scalars", "px_n_e", sc["px_n_e"], len(m.px))
        node = img["px_node"].tolist()
        assert len(node) == len(img["px_key"]), (ctx, "px", "lengths of the two arrays", len(node), len(img["px_key"]))
        for i in range(1, len(node)):
            a, b = (m.term_of(x) if x < m.n else None for x in node[i - 1:i + 1])
            assert a is not None and b is not None and a < b, (ctx, "px_node", "index", i, "term", b, "is not above its predecessor", a)
        _same(ctx, "px_node", node, m.px)
        _same(ctx, "px_key", img["px_key"], m.px_key)


# ---------------------------------------------------------------------------------------------------
# the corpus
# ---------------------------------------------------------------------------------------------------

def _words(rng, n, alphabet, lo, hi, taken):
    out = []
    while len(out) < n:
        w = bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))
        if w not in taken:
            taken.add(w)
            out.append(w)
    return out


N_DEAD, N_LIVE0 = 1250, 257     # terms whose docs are gone before the first load; live terms at the first load


def corpus():
    """-> (events, cut, zero, info).  events[:cut[k]] is snapshot k (nxsfmt.build_images_log), zero[k] the terms
    whose on-disk total is written as 0 at snapshot k (set_totals), info the designed terms by name.

    The root R has 40 bytes over a-f, so every short term hangs 30 to 40 slots below it, R + tail hangs in slot
    len(tail), and a term over u-z of 64 bytes or more is 63 or more away: the clamped slot.
      lengths     g (1), orderab (7), orderabc (8), orderabcd (9), q8r8 (16), q8r8 + s / t (17), R + 24 / 25 / 26 /
                  27 bytes (64 .. 67, reached by the walk), XL (300, below slot 63)
      bytes       \\x7fabc < \\x80abc < \\xffz only when bytes compare unsigned; a\\x80, a\\xff; ABBA / abba and
                  \\xe1\\xe2 / AB collide under & 31
      order       ordera is a proper prefix of orderab ...; chunk000A / chunk000B differ first in byte 8, q8r8s /
                  q8r8t in byte 16 (q8r8 itself ends at the chunk's edge)
      slot 63     T (65 bytes over u-z), T1 = T[:64] + one other byte, T2 = T[:64], XL: all live
      flag / df   ghost: total 0 on disk from the start, live; dead1: its only doc goes at snapshot 1, the total stays
                  above 0 (flag 1, df 0) and a doc of snapshot 2 brings it back; gone: its only doc goes at
                  snapshot 1 and its total is written as 0 from then on (the flag moves)
      df order    swa (df 3) and swb (df 2); snapshot 2 appends two docs with swb
      sizes       1250 terms live only in docs that are removed before the first load (flag 1, df 0); 257 live terms
                  at the first load, 255 after snapshot 1, 256 after snapshot 2 (the order's entries; suggest's
                  candidates are two fewer: R + 27 bytes and XL are too long)
    Snapshots: 0 the first load; 1 removals only; 2 appends without a new term; 3 appends with new terms, one of
    them R[:39]: one edit from the root, its lowest slot by far, so BFS numbers it 1 and moves every other node; 4 a
    doc whose id lies below the highest loaded one: the full rebuild."""
    rng = random.Random(6601)
    af, uz = b"abcdef", b"uvwxyz"
    R = bytes(rng.choice(af) for _ in range(40))
    T = bytes(rng.choice(uz) for _ in range(65))
    info = {"R": R, "T": T, "T1": T[:64] + (b"u" if T[64:] != b"u" else b"v"), "T2": T[:64],
            "XL": bytes(rng.choice(uz) for _ in range(300)),
            "L64": R + bytes(rng.choice(af) for _ in range(24)), "L65": R + bytes(rng.choice(af) for _ in range(25)),
            "L66": R + bytes(rng.choice(af) for _ in range(26)), "L67": R + bytes(rng.choice(af) for _ in range(27)),
            "ghost": b"ghost", "dead1": b"deadone", "gone": b"goneterm", "swa": b"swa", "swb": b"swb",
            "newlow": R[:39], "new": [b"newterma", b"newtermb", b"\xf0new"], "rebuilt": b"rebuilt"}
    designed = [R, b"g", b"ordera", b"orderab", b"orderabc", b"orderabcd", b"chunk000A", b"chunk000B",
                b"qqqqqqqqrrrrrrrr", b"qqqqqqqqrrrrrrrrs", b"qqqqqqqqrrrrrrrrt",
                info["L64"], info["L65"], info["L66"], info["L67"], T, info["T1"], info["T2"], info["XL"],
                b"\x7fabc", b"\x80abc", b"\xffz", b"a\x80", b"a\xff", b"ABBA", b"abba", b"\xe1\xe2", b"AB",
                info["ghost"], info["swa"], info["swb"], b"all"]
    solo = [info["dead1"], info["gone"]]                # live at the first load, each in a doc of its own
    taken = set(designed) | set(solo) | {info["newlow"], info["rebuilt"]} | set(info["new"])
    live = designed + _words(rng, N_LIVE0 - len(designed) - len(solo), af, 2, 10, taken)
    dead = _words(rng, N_DEAD, af, 2, 10, taken)
    info["live0"], info["dead"] = live + solo, dead
    ev = [("add", 5, [R, b"all"])]
    for j in range(50):                                  # the docs that are gone before the first load
        ev.append(("add", 10 + 10 * j, dead[25 * j:25 * j + 25]))
    nd = 150
    docs = [[b"all"] for _ in range(nd)]
    for i, t in enumerate(live):
        df = {info["swa"]: 3, info["swb"]: 2}.get(t, 1 + i % 5)
        if t not in (R, b"all"):
            for s in range(df):
                docs[(i + 17 * s) % nd].append(t)
    for j in range(nd):
        ev.append(("add", 1000 + 10 * j, docs[j]))
    ev += [("add", 5000, [b"all", info["dead1"]]), ("add", 5010, [b"all", info["gone"]])]
    ev += [("rm", 10 + 10 * j) for j in range(50)]
    cut = [len(ev)]
    ev += [("rm", 5000), ("rm", 5010)]
    cut.append(len(ev))
    ev += [("add", 6000, [b"all", info["swb"]]), ("add", 6010, [b"all", info["swb"], info["dead1"]])]
    cut.append(len(ev))
    ev += [("add", 6100, [b"all", info["newlow"], info["new"][0]]), ("add", 6110, [b"all", info["new"][1], info["new"][2], info["new"][0]])]
    cut.append(len(ev))
    ev += [("add", 15, [b"all", info["rebuilt"], b"g"])]
    cut.append(len(ev))
    zero = [{info["ghost"]}] + [{info["ghost"], info["gone"]}] * 4
    return ev, cut, zero, info


def images(ev, zero):
    """the two files of one snapshot"""
    import nxsfmt
    timg, dimg, _ = nxsfmt.build_images_log(ev)
    return set_totals(timg, {t: 0 for t in zero}), dimg


def live_df(ev):
    """{term bytes: the number of live docs that hold it}, from the events alone"""
    docs = {}
    for e in ev:
        if e[0] == "add":
            docs[e[1]] = set(e[2])
        else:
            del docs[e[1]]
    df = {}
    for toks in docs.values():
        for t in toks:
            df[t] = df.get(t, 0) + 1
    return df


def event_models(ev, cut, zero):
    """the models of all snapshots from the events alone (totals: as images() writes them; df: live_df)"""
    out = []
    for k in range(len(cut)):
        terms, totals = read_terms(images(ev[:cut[k]], zero[k])[0])
        df = live_df(ev[:cut[k]])
        out.append(TermModel(terms, totals, [df.get(t, 0) for t in terms]))
    return out


def preconditions(models, info):
    """Every designed edge, at the snapshot that needs it, from the models of the five snapshots alone."""
    m0 = models[0]
    live_len = lambda m: {len(m.term_of(i)) for i in m.px}
    for m in models:
        assert m.terms[0] == info["R"] and m.node_term[0] == 0
        assert {1, 7, 8, 9, 16, 17, 64, 65, 66, 67, 300} <= live_len(m)
        fz_len = {len(m.term_of(i)) for i in m.fz}
        assert {64, 65, 66} <= fz_len and max(fz_len) == 66                  # reached by the walk, up to FZ_MAXLEN
        assert max(len(m.term_of(i)) for i in m.sg) == 66 and m.node_of(info["L67"]) in m.px
        # the slot-63 subtree: not among the match-first candidates, among suggest's and in the order
        t = m.node_of(info["T"])
        assert m.parent[t] == 0 and m.slot[t] == 63
        for name in ("T", "T1", "T2", "XL"):
            i = m.node_of(info[name])
            assert m.cut[i] and m.bk["flags"][i] & 1 and i not in m.fz and i in m.px, name
            assert (i in m.sg) == (name != "XL"), name
        assert m.slot[m.node_of(info["XL"])] == 63 and m.parent[m.node_of(info["XL"])] == t
        # unsigned order, prefixes, chunk edges: neighbours in the order
        pos = {m.term_of(i): k for k, i in enumerate(m.px)}
        assert pos[b"\x7fabc"] < pos[b"\x80abc"] < pos[b"\xffz"] == len(m.px) - 1
        assert pos[b"a\x80"] + 1 == pos[b"a\xff"] and pos[b"abba"] < pos[b"a\x80"]
        assert pos[b"ordera"] + 1 == pos[b"orderab"] and pos[b"orderab"] + 1 == pos[b"orderabc"] == pos[b"orderabcd"] - 1
        assert pos[b"chunk000A"] + 1 == pos[b"chunk000B"]
        assert pos[b"qqqqqqqqrrrrrrrr"] + 2 == pos[b"qqqqqqqqrrrrrrrrs"] + 1 == pos[b"qqqqqqqqrrrrrrrrt"]
        assert signature(b"ABBA") == signature(b"abba") and signature(b"\xe1\xe2") == signature(b"AB")
        # flag 0 and live: ghost
        g = m.node_of(info["ghost"])
        assert m.totals[m.node_term[g]] == 0 and g not in m.fz and g in m.sg and g in m.px
    # sizes: the order's entries at 257, 255, 256; suggest's candidates start at 255; the grids over n_bk and n_fz
    # have several blocks and a last one that is not full
    assert [len(m.px) for m in models[:3]] == [257, 255, 256], [len(m.px) for m in models]
    assert len(m0.sg) == 255 and all(len(m.sg) == len(m.px) - 2 for m in models)
    assert all(m.n > 1024 and m.n % 256 and len(m.fz) % 256 for m in models)
    # snapshot 1: removals only -- gone loses flag and df, dead1 the df alone; the numbering stays
    m1 = models[1]
    assert m1.terms == m0.terms and np.array_equal(m1.bk["term_id"], m0.bk["term_id"])
    for name, flag in (("gone", 0), ("dead1", 1)):
        i = m0.node_of(info[name])
        assert m0.bk["flags"][i] == 1 and i in m0.px and m1.bk["flags"][i] == flag and i not in m1.px and i not in m1.sg, name
        assert (i in m1.fz) == bool(flag), name
    # snapshot 2: no new term, no flag moves, swb overtakes swa, dead1 is back
    m2 = models[2]
    assert m2.terms == m1.terms and np.array_equal(m2.bk, m1.bk)
    dfo = lambda m, name: m.dfs[m.terms.index(info[name])]
    assert dfo(m1, "swa") > dfo(m1, "swb") and dfo(m2, "swa") < dfo(m2, "swb")
    assert m2.node_of(info["dead1"]) in m2.px and not np.array_equal(m2.px_key[:len(m1.px_key)], m1.px_key)
    # snapshot 3: new terms; R[:39] is node 1 and most nodes move
    m3 = models[3]
    assert len(m3.terms) == len(m2.terms) + 4 and m3.node_of(info["newlow"]) == 1 and m3.slot[1] == 1
    moved = sum(1 for i in range(m2.n) if m3.bk["term_id"][i] != m2.bk["term_id"][i])
    assert moved > m2.n * 9 // 10, moved
    # snapshot 4: one more term
    assert len(models[4].terms) == len(m3.terms) + 1
