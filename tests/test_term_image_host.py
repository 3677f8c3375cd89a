"""CPU tier for the term-image tests: the host model of tests/term_truth.py against the library's host flatten
and the oracle's BK-tree, the corpus's designed edges, and the checker itself -- it accepts the images the model
stands for and names a single wrong value in every array.  A GPU test whose checker cannot fail proves nothing, and
no mutated library is ever run on a GPU (a wrong image can make the scans read out of bounds): these mutations of
an IMAGE are the evidence that check_term_image bites."""
import random

import numpy as np
import pytest

import nxsearch_amd as N
import oracle_lib as O
import term_truth as TT


@pytest.fixture(scope="module")
def snaps():
    ev, cut, zero, info = TT.corpus()
    return TT.event_models(ev, cut, zero), info


def random_dict(seed):
    rng = random.Random(seed)
    alphabet = [b"abcd", b"abcdefghijklmnopqrstuvwxyz", bytes(range(0x7e, 0x86)) + b"\xff"][seed % 3]
    words = TT._words(rng, 300, alphabet, 1, 12, set())
    words += [bytes(rng.choice(alphabet) for _ in range(n)) for n in (63, 64, 65, 66, 67, 130)]
    return words


def test_preconditions_hold_for_the_corpus(snaps):
    models, info = snaps
    TT.preconditions(models, info)


def test_model_nodes_equal_the_host_flatten(snaps):
    """The model's tree -- its own Levenshtein, slot clamp, BFS numbering -- against nxs_bk_build + nxs_bk_flatten
    (N.bk_image): every field of every node, the bytes and the depth, on the dictionaries of the five snapshots
    and on three random ones (a 4-letter alphabet: deep chains; 26 letters; bytes around 0x80 and 0xff)."""
    models, _ = snaps
    dicts = [m.terms for m in models] + [random_dict(s) for s in (3, 4, 5)]
    for words in dicts:
        m = TT.TermModel(words, [1] * len(words), [1] * len(words))      # (the hook writes every flag as 1)
        nodes, depth = N.bk_image(words)
        assert len(nodes) == m.n and depth == m.depth
        for i, nd in enumerate(nodes):
            want = m.bk[i]
            got = (nd["bitmap"], nd["first_child"], nd["term_id"], nd["term"], nd["flags"], nd["inl"])
            assert got == (int(want["bitmap"]), int(want["first_child"]), int(want["term_id"]), m.term_of(i), 1,
                           bytes(want["inl"])), (i, got)


M64 = (1 << 64) - 1


def _walk(m, q, tol=2):
    """bktree_search over the model's image, level by level (tests/test_host_logic.py::_image_search, here also for
    tokens more than 63 edits from a node) -> (matches in BFS order, nodes visited)"""
    frontier, out, visited = [0], [], 0
    while frontier:
        nxt = []
        for i in frontier:
            d = O.levdist(q, m.term_of(i))
            visited += 1
            if d <= tol:
                out.append(i)
            bm, first = int(m.bk["bitmap"][i]), int(m.bk["first_child"][i])
            # slots [d - tol, min(d + tol, 63)), as two 64-bit masks whose shift counts wrap at 64 (the reference's
            # arithmetic, k_bk_level / k_fz_chain): for d - tol >= 64 the lower end comes around
            lo = (M64 << ((d - tol if d > tol else 0) & 63)) & M64
            hi = M64 >> ((64 - min(d + tol, 63)) & 63)
            for slot in range(63):
                if (bm & lo & hi) >> slot & 1:
                    nxt.append(first + bin(bm & ((1 << slot) - 1)).count("1"))
        frontier = nxt
    return out, visited


def test_model_tree_gives_the_oracles_visit_counts_and_match_order(snaps):
    """O.BKTree (pinned to the genuine bktree.c) over the same words: the same number of nodes visited and the same
    matches in the same order; and the model's distance is the oracle's."""
    models, info = snaps
    rng = random.Random(77)
    for words in (models[3].terms, random_dict(3), random_dict(5)):
        m = TT.TermModel(words, [1] * len(words), [1] * len(words))
        orc = O.BKTree(words)
        qs = [bytearray(rng.choice(words)) for _ in range(80)]
        for q in qs:
            q[rng.randrange(len(q))] = rng.choice(b"abcdefuvw\x80")
        for q in [bytes(q) for q in qs] + [info["T2"], info["L66"][:-1], info["R"][:39]]:
            res, nvis = orc.search(q, 2)
            got, gvis = _walk(m, q, 2)
            assert gvis == nvis and [m.node_term[i] for i in got] == res, q
        for _ in range(300):
            a, b = rng.choice(words), rng.choice(words)
            assert TT.levdist(a, b) == O.levdist(a, b), (a, b)
        orc.close()


def test_checker_accepts_the_models_own_images(snaps):
    """every part, at every snapshot and on the three tiny shapes (no node at all included)"""
    models, _ = snaps
    tiny = [TT.TermModel([], [], []), TT.TermModel([b"one"], [2], [1]), TT.TermModel([b"one", b"two"], [2, 0], [0, 0])]
    for k, m in enumerate(models + tiny):
        img = TT.image_of(m, sg_gen=3 + k, px_gen=5 + k, px_builds=k + 1)
        TT.check_term_image(img, m, k)
        for parts in (("bk",), ("bk", "fz"), ("bk", "fz", "sg"), ("px",)):
            TT.check_term_image(img, m, k, parts=parts)


# ---- one value at a time ---------------------------------------------------------------------

def _flag(img, m, prev, info):
    i = m.node_of(info["dead1"])
    img["bk"]["flags"][i] ^= 1
    return "bk.flags", i


def _first_child(img, m, prev, info):
    i = m.n // 2
    img["bk"]["first_child"][i] += 1
    return "bk.first_child", i


def _parent(img, m, prev, info):
    i = m.n - 7
    img["bk_parent"][i] -= 1                    # off by one node: only a distance-2 match below it walks there
    return "bk_parent", i


def _slot(img, m, prev, info):
    i = m.n - 7
    img["bk_slot"][i] += 1
    return "bk_slot", i


def _sig_bit_dropped(img, m, prev, info):
    i = len(m.fz) // 3
    img["fz_sig"][i] &= img["fz_sig"][i] - 1
    return "fz_sig", i, "bits missing"


def _sig_bit_added(img, m, prev, info):
    i = len(m.sg) // 3
    img["sg_sig"][i] |= 1 << 29                 # no term of the corpus holds a byte with (b & 31) == 29
    return "sg_sig", i, "bits too many"


def _slot63_candidate(img, m, prev, info):
    t2 = m.node_of(info["T2"])                  # 64 bytes: its place is before the first 65-byte candidate
    i = int(m.fz_len_start[65])
    for name in ("fz_node", "fz_sig", "fz_len"):
        extra = {"fz_node": t2, "fz_sig": TT.signature(info["T2"]), "fz_len": 64}[name]
        img[name] = np.insert(img[name], i, extra)
    img["fz_len_start"][65:] += 1
    return "fz_node", i, "hangs below a slot-63 child"


def _len_start(img, m, prev, info):
    img["fz_len_start"][9] += 1
    return "fz_len_start", 9


def _order_swapped(img, m, prev, info):
    i = len(m.px) // 2
    for name in ("px_node", "px_key"):
        img[name][[i, i + 1]] = img[name][[i + 1, i]]
    return "px_node", i + 1, "is not above its predecessor"


def _key_with_the_old_df(img, m, prev, info):
    i = [m.term_of(x) for x in m.px].index(info["swb"])
    j = [prev.term_of(x) for x in prev.px].index(info["swb"])
    assert prev.px_key[j] != m.px_key[i]
    img["px_key"][i] = prev.px_key[j]
    return "px_key", i


MUTATIONS = [_flag, _first_child, _parent, _slot, _sig_bit_dropped, _sig_bit_added, _slot63_candidate, _len_start,
             _order_swapped, _key_with_the_old_df]


@pytest.mark.parametrize("mutate", MUTATIONS, ids=[f.__name__[1:] for f in MUTATIONS])
def test_checker_names_one_wrong_value(snaps, mutate):
    """Snapshot 2 (the df of swb has just moved), one value changed in the image the model stands for: the
    checker fails, and its message names the array and the index (NOTES.md has the table)."""
    models, info = snaps
    m, prev = models[2], models[1]
    img = TT.image_of(m)
    TT.check_term_image(img, m, "clean")
    part, index, *words = mutate(img, m, prev, info)
    with pytest.raises(AssertionError) as e:
        TT.check_term_image(img, m, "mutated")
    msg = e.value.args[0]
    assert msg[0] == "mutated" and msg[1] == part and msg[2] == "index" and msg[3] == index, msg
    for w in words:
        assert w in msg, msg
