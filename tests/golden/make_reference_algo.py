#!/usr/bin/env python3
"""Records the reference's answers for the seeded inputs of
tests/test_oracle_vs_reference.py into tests/golden/reference_algo.json.gz.

Needs oracle/_ref/libnxsref.so: the reference's src/algo/{levdist,bktree,deque,
heap}.c compiled in place by oracle/Makefile from a reference checkout.  Only
DATA is recorded (distances, result ids, visit counts, top-k pairs), no source
text; the file it writes is committed, so the tests need no reference checkout.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import oracle_lib as O                                  # noqa: E402
import test_oracle_vs_reference as T                    # noqa: E402


def main():
    R = O.ref()
    if R is None:
        sys.exit("oracle/_ref/libnxsref.so is not built (oracle/Makefile needs the reference checkout)")
    out = {"_comment": "answers of the reference's src/algo/{levdist,bktree,heap}.c (oracle/_ref) for the seeded "
                       "inputs of tests/test_oracle_vs_reference.py; written by tests/golden/make_reference_algo.py"}
    out["levdist"] = [R.ref_levdist(a, len(a), b, len(b)) for a, b in T.levdist_pairs()]
    out["bktree"] = {}
    for seed, n, alphabet in T.BKTREE_SETS:
        words, searches = T.bktree_set(seed, n, alphabet)
        tree = O.RefBKTree(words)
        out["bktree"][str(seed)] = T.bk_answers(tree, searches)
        tree.close()
    words, queries = T.long_words_set()
    tree = O.RefBKTree(words)
    out["bktree_long_words"] = T.bk_answers(tree, [(q, 2) for q in queries])
    tree.close()
    out["topk"] = [T.topk_answer(ids, sc, k) for ids, sc, k in T.topk_trials()]
    data = json.dumps(out, separators=(",", ":")).encode()
    with open(T.GOLDEN, "wb") as f:
        # mtime 0: the same answers give the same bytes
        f.write(gzip.compress(data, compresslevel=9, mtime=0))


if __name__ == "__main__":
    main()
