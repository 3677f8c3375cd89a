#!/usr/bin/env python3
"""What the related terms of a query's matches cost.

On the C3 corpus (10M docs / 1M terms; DOCS / TERMS override), with profiling on: Index.related (nxsgpu_related)
for batches of 1, 8, 32 and 256 C3 queries (5 terms, half AND, half OR) at k = 8 -- STEPS calls per setting give
the HIP-event ms of k_rt_mask, k_rt_scan, k_rt_select and k_rt_merge per call and per pass (a pass serves a group
of at most 32 plans and streams the posting array once), the wall-clock ms of the call and the mean doc-set size
--, then one selective query (a 5-term AND) against one broad query (a 5-term OR) alone, and the host route
(NXS_GPU_RELATED=host: the posting array copied back, a plain loop on one host thread) beside the batches of 1
and 8 (HOST_N) for the same queries, HOST_STEPS calls each (HOST=0 skips it).  `post_dt_bytes` is what k_rt_scan reads once
per pass: compare scan_ms_per_pass with tools/stream_probe.hip reading that many bytes in the same session.

The host route copies d_post_dt back into pageable host memory on EVERY call (8 B a posting) and walks every
list once per query: mind the box's free memory, or set HOST=0.

These figures are a record, not a verdict.  Reads nothing but its own corpus.  Prints one JSON line; OUT=path
writes it there too (default profiles/related_probe.json), stamped with the source hash bench.py uses."""
import hashlib
import json
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nxsearch_amd as N
from nxsearch_amd import corpus

DOCS = int(os.environ.get("DOCS", 10_000_000))
TERMS = int(os.environ.get("TERMS", 1_000_000))
STEPS = max(2, int(os.environ.get("STEPS", 5)))
HOST_STEPS = max(1, int(os.environ.get("HOST_STEPS", 1)))
K = int(os.environ.get("K", 8))
HOST_N = [int(x) for x in os.environ.get("HOST_N", "1,8").split(",")]   # of 1, 8, 32, 256
work = os.environ.get("WORK", "/dev/shm/nxs_related_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "related_probe.json"))


def source_hash():
    """(= bench.py's)"""
    root = os.path.join(ROOT, "nxsearch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def timed(idx, qs, steps):
    """steps calls of Index.related -> (the figures per call and per pass, the last answer)"""
    idx.related_profile(reset=True)
    wall, got = [], None
    for _ in range(steps):
        t0 = time.perf_counter()
        got = idx.related(qs, limit=K, fuzzymatch=False)
        wall.append(1e3 * (time.perf_counter() - t0))
    p = idx.related_profile(reset=True)
    n, passes = float(steps), float(max(p["passes"], 1))
    ok = [g for g in got if not isinstance(g, Exception)]
    r = {"wall_ms": round(statistics.median(wall), 3), "calls": steps, "passes_per_call": p["passes"] / n,
         "plans_per_call": (p["device_queries"] + p["host_queries"]) / n,
         "mean_docs": round(sum(g.docs for g in ok) / float(max(len(ok), 1)), 1),
         "mean_matches": round(sum(g.matches for g in ok) / float(max(len(ok), 1)), 1)}
    for k in ("mask", "scan", "select", "merge"):
        r["k_rt_%s_ms" % k] = round(p[k + "_ms"] / n, 4)
        r["k_rt_%s_ms_per_pass" % k] = round(p[k + "_ms"] / passes, 4)
    return r, got


def main():
    res = {"what": "related terms: HIP-event ms of nxsgpu_related's kernels per call and per pass at k = %d (mean of %d "
                   "calls), wall-clock ms (median), the host route beside it" % (K, STEPS),
           "source_hash": source_hash(), "docs": DOCS, "terms": TERMS, "k": K}
    os.makedirs(work, exist_ok=True)
    c = corpus.write_corpus(work, DOCS, TERMS, seed=0)
    terms = corpus.term_strings(TERMS, seed=0)
    nxs = N.Nxs(work)
    idx = nxs.open_files(c["terms"], c["dtmap"], algo="BM25")
    res["post_dt_bytes"] = 8 * int(N.lib().nxsgpu_index_postings(idx.device))
    idx.set_profiling(True)
    qs = corpus.queries_bool5(terms, 256, seed=21)
    idx.related(qs[:1], limit=K, fuzzymatch=False)      # (the pass's stream, events and workspace come with the first call)
    device = {}
    for n in (1, 8, 32, 256):
        res["device_%d" % n], device[n] = timed(idx, qs[:n], STEPS)
    res["selective_and"], _ = timed(idx, [qs[0]], STEPS)
    res["broad_or"], _ = timed(idx, [qs[1]], STEPS)
    if os.environ.get("HOST", "1") != "0":
        os.environ["NXS_GPU_RELATED"] = "host"
        idx.reconfigure()
        for n in HOST_N:
            r, got = timed(idx, qs[:n], HOST_STEPS)
            res["host_%d" % n] = {"wall_ms": r["wall_ms"], "calls": HOST_STEPS,
                                  "equal": got == device[n] and [g.docs for g in got] == [g.docs for g in device[n]]}
        del os.environ["NXS_GPU_RELATED"]
        idx.reconfigure()
    else:
        res["host"] = "not run"
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
