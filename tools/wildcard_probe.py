#!/usr/bin/env python3
"""What wildcard matching costs: the pass per kernel, per pattern shape, with the host route for scale.

On the C4 dictionary (10M docs / 1M terms; DOCS / TERMS override) patterns are cut out of C4's own tokens
(corpus.queries_fuzzy), PATTERNS (64) per pass, k = 8 and 32, in four shapes: leading star (`*tail`: the whole
order is scanned), infix (`*mid*`), head + tail (`he*il`: the range of a two-byte head) and `?` (one byte of the
token replaced: the range of the head in front of it, the length filter).  With profiling on, STEPS passes per
setting give the HIP-event ms of the range searches, k_wc_match and k_wc_merge and of the pass, and the mean and
largest `matches`.  The host route (NXS_GPU_WILDCARD=host: nxs_wild_rank, a linear scan on one core) answers
HOST_PATTERNS (8) of the same patterns in the same run, wall clock.

There is no parent to compare with: the figures are a record, not a verdict.  Reads nothing but its own corpus.
Prints one JSON line; OUT=path writes it there too (default profiles/wildcard_probe.json), stamped with the
source hash bench.py uses."""
import hashlib
import json
import os
import shutil
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nxsearch_amd as N
from nxsearch_amd import corpus

DOCS = int(os.environ.get("DOCS", 10_000_000))
TERMS = int(os.environ.get("TERMS", 1_000_000))
PATTERNS = int(os.environ.get("PATTERNS", 64))
HOST_PATTERNS = int(os.environ.get("HOST_PATTERNS", 8))
STEPS = max(3, int(os.environ.get("STEPS", 10)))
work = os.environ.get("WORK", "/dev/shm/nxs_wildcard_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "wildcard_probe.json"))


def source_hash():
    """(= bench.py's)"""
    root = os.path.join(ROOT, "nxsearch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def shapes(toks):
    toks = [t for t in toks if len(t) >= 5 and b"*" not in t and b"?" not in t]
    return {
        "leading_star": [b"*" + t[-3:] for t in toks],
        "infix": [b"*" + t[1:4] + b"*" for t in toks],
        "head_tail": [t[:2] + b"*" + t[-2:] for t in toks],
        "question": [t[:2] + b"?" + t[3:] for t in toks],
    }


def main():
    res = {"what": "wildcard matching: HIP-event ms per pass of %d patterns (mean of %d passes); host route: wall ms "
                   "per pattern over %d patterns" % (PATTERNS, STEPS, HOST_PATTERNS),
           "source_hash": source_hash(), "patterns": PATTERNS, "docs": DOCS, "terms": TERMS,
           "date": time.strftime("%Y-%m-%d")}
    os.makedirs(work, exist_ok=True)
    c = corpus.write_corpus(work, DOCS, TERMS, seed=7)
    terms = corpus.term_strings(TERMS, seed=7)
    toks = [t if isinstance(t, bytes) else t.encode() for t in corpus.queries_fuzzy(terms, 4 * PATTERNS, seed=4)]
    nxs = N.Nxs(work)
    idx = nxs.open_files(c["terms"], c["dtmap"])
    t0 = time.perf_counter()
    idx.wildcard([b"a*a"], limit=5)             # builds the order
    p = idx.wildcard_profile()
    res["first_call_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    res["entries"], res["parts"] = p["entries"], int(os.environ.get("NXS_GPU_WILD_PARTS", 64))
    idx.set_profiling(True)
    idx.wildcard([b"a*a"], limit=5)             # (the pass's events are created by the first profiled call)
    for name, pats in shapes(toks).items():
        pats = pats[:PATTERNS]
        for k in (8, 32):
            idx.wildcard_profile(reset=True)
            got = None
            for _ in range(STEPS):
                got = idx.wildcard(pats, limit=k)
            p = idx.wildcard_profile(reset=True)
            n = float(max(p["passes"], 1))
            res["%s_k%d" % (name, k)] = {
                "pass_ms": round(p["ms"] / n, 4), "range_ms": round(p["range_ms"] / n, 4),
                "k_wc_match_ms": round(p["match_ms"] / n, 4), "k_wc_merge_ms": round(p["merge_ms"] / n, 4),
                "passes": p["passes"], "n": len(pats),
                "mean_matches": round(sum(g.matches for g in got) / float(len(got)), 1),
                "max_matches": max(g.matches for g in got)}
        # the host route, for scale
        os.environ["NXS_GPU_WILDCARD"] = "host"
        idx.reconfigure()
        idx.wildcard(pats[:1], limit=8)         # (the host copy of the dictionary)
        t0 = time.perf_counter()
        host = idx.wildcard(pats[:HOST_PATTERNS], limit=8)
        res["%s_host_ms_per_pattern" % name] = round(1e3 * (time.perf_counter() - t0) / max(len(host), 1), 3)
        del os.environ["NXS_GPU_WILDCARD"]
        idx.reconfigure()
        assert [list(g) for g in host] == [list(g) for g in idx.wildcard(pats[:HOST_PATTERNS], limit=8)]
    idx.set_profiling(False)
    idx.close()
    nxs.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")
    if not os.environ.get("KEEP"):
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
