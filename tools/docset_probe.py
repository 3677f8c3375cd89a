#!/usr/bin/env python3
"""What a search within a doc-id set costs.

On the C3 corpus (10M docs / 1M terms; DOCS / TERMS override), with profiling on: Index.search_docs
(nxsgpu_search_docs) for a batch of NQ (32) C3 queries (5 terms, half AND, half OR) at limit 10 against ONE shared set
of 1 k, 64 k and 1 M random doc ids (SETS) -- STEPS calls per set size give the HIP-event ms of k_ds_ord, k_ds_score
and the replay per call, the wall-clock ms of the call (sorting the set on the host included) and the candidates --,
the host route (NXS_GPU_DOCSET=host: the index arrays copied back, nxs_ds_lane on one host thread, the same device
replay) beside the sizes in HOST_SETS, HOST_STEPS calls each (HOST=0 skips it), and an unrestricted top-10
search_batch of the same queries for scale.  `crossover_docs` is where the doc-driven kernels' time, read as a
straight line between the two measured sizes that bracket it, meets the unrestricted batch's device time: beyond that
many docs a set is cheaper to serve from the lists (None: the smallest set is already dearer).

The host route copies 16 B a posting and 8 B a doc back into pageable host memory on EVERY call: mind the box's free
memory, or set HOST=0.

These figures are a record, not a verdict.  Reads nothing but its own corpus.  Prints one JSON line; OUT=path writes
it there too (default profiles/docset_probe.json), stamped with the source hash bench.py uses."""
import hashlib
import json
import os
import shutil
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nxsearch_amd as N
from nxsearch_amd import corpus

DOCS = int(os.environ.get("DOCS", 10_000_000))
TERMS = int(os.environ.get("TERMS", 1_000_000))
STEPS = max(2, int(os.environ.get("STEPS", 5)))
HOST_STEPS = max(1, int(os.environ.get("HOST_STEPS", 1)))
NQ = int(os.environ.get("NQ", 32))
LIMIT = int(os.environ.get("LIMIT", 10))
SETS = [int(x) for x in os.environ.get("SETS", "1000,65536,1000000").split(",")]
HOST_SETS = [int(x) for x in os.environ.get("HOST_SETS", "1000,65536").split(",")]
work = os.environ.get("WORK", "/dev/shm/nxs_docset_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "docset_probe.json"))


def source_hash():
    """(= bench.py's)"""
    root = os.path.join(ROOT, "nxsearch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def timed(idx, qs, ids, steps):
    """steps calls of Index.search_docs -> (the figures per call, the last answer)"""
    idx.search_docs_profile(reset=True)
    wall, got = [], None
    for _ in range(steps):
        t0 = time.perf_counter()
        got = idx.search_docs(qs, ids, limit=LIMIT, fuzzymatch=False, total=True)
        wall.append(1e3 * (time.perf_counter() - t0))
    p = idx.search_docs_profile(reset=True)
    n = float(steps)
    ok = [g for g in got if not isinstance(g, Exception)]
    r = {"wall_ms": round(statistics.median(wall), 3), "calls": steps, "passes_per_call": p["passes"] / n,
         "cells_per_call": (p["device_cells"] + p["host_cells"]) / n, "candidates_per_call": p["candidates"] / n,
         "mean_total": round(sum(g.total for g in ok) / float(max(len(ok), 1)), 1)}
    for k in ("ord", "score", "replay"):
        r["k_ds_%s_ms" % k if k != "replay" else "k_replay_ms"] = round(p[k + "_ms"] / n, 4)
    r["kernels_ms"] = round((p["ord_ms"] + p["score_ms"] + p["replay_ms"]) / n, 4)
    return r, got


def main():
    res = {"what": "search within a doc-id set: HIP-event ms of nxsgpu_search_docs' kernels per call for %d C3 queries on "
                   "one shared set at limit %d (mean of %d calls), wall-clock ms (median), the host route and an "
                   "unrestricted top-%d batch beside it" % (NQ, LIMIT, STEPS, LIMIT),
           "source_hash": source_hash(), "docs": DOCS, "terms": TERMS, "queries": NQ, "limit": LIMIT}
    os.makedirs(work, exist_ok=True)
    c = corpus.write_corpus(work, DOCS, TERMS, seed=0)
    terms = corpus.term_strings(TERMS, seed=0)
    nxs = N.Nxs(work)
    idx = nxs.open_files(c["terms"], c["dtmap"], algo="BM25")
    res["postings"] = int(N.lib().nxsgpu_index_postings(idx.device))
    idx.set_profiling(True)
    qs = [q.decode() if isinstance(q, bytes) else q for q in corpus.queries_bool5(terms, NQ, seed=21)]
    rng = np.random.default_rng(7)
    sets = {n: rng.choice(np.arange(1, DOCS + 1, dtype=np.uint64), size=min(n, DOCS), replace=False) for n in sorted(set(SETS + HOST_SETS))}
    idx.search_docs(qs[:1], sets[min(sets)], limit=LIMIT, fuzzymatch=False)     # (stream, events and workspace come with the first call)
    device = {}
    for n in SETS:
        res["device_%d" % n], device[n] = timed(idx, qs, sets[n], STEPS)
    # the unrestricted batch of the same queries
    idx.search_batch(qs, limit=LIMIT, fuzzymatch=False)
    idx.profile(reset=True)
    wall = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        idx.search_batch(qs, limit=LIMIT, fuzzymatch=False)
        wall.append(1e3 * (time.perf_counter() - t0))
    p = idx.profile(reset=True)
    res["unrestricted"] = {"wall_ms": round(statistics.median(wall), 3), "calls": STEPS,
                           "scan_ms": round(p["scan_ms"] / STEPS, 4), "replay_ms": round(p["replay_ms"] / STEPS, 4),
                           "kernels_ms": round((p["scan_ms"] + p["replay_ms"]) / STEPS, 4)}
    # where the doc-driven kernels' time, read as a straight line between two measured sizes, meets the unrestricted
    # batch's: between the pair that brackets it, else on the line through the two largest sizes
    sizes = sorted(SETS)
    ms = [res["device_%d" % n]["kernels_ms"] for n in sizes]
    want = res["unrestricted"]["kernels_ms"]
    if len(sizes) >= 2:
        res["ms_per_million_docs"] = round(1e6 * (ms[-1] - ms[-2]) / float(sizes[-1] - sizes[-2]), 4)
        pair = next((i for i in range(len(sizes) - 1) if ms[i] <= want < ms[i + 1]), len(sizes) - 2)
        slope = (ms[pair + 1] - ms[pair]) / float(sizes[pair + 1] - sizes[pair])
        res["crossover_docs"] = int(sizes[pair] + (want - ms[pair]) / slope) if slope > 0 and want >= ms[0] else None
    if os.environ.get("HOST", "1") != "0":
        os.environ["NXS_GPU_DOCSET"] = "host"
        idx.reconfigure()
        for n in HOST_SETS:
            r, got = timed(idx, qs, sets[n], HOST_STEPS)
            res["host_%d" % n] = {"wall_ms": r["wall_ms"], "calls": HOST_STEPS, "k_replay_ms": r["k_replay_ms"],
                                  "equal": n in device and got == device[n] and [g.total for g in got] == [g.total for g in device[n]]}
        del os.environ["NXS_GPU_DOCSET"]
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
