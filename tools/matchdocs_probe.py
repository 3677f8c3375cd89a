#!/usr/bin/env python3
"""What listing a query's matches by doc id costs.

On the C3 corpus (10M docs / 1M terms; DOCS / TERMS override), with profiling on: nxs_index_match_docs_batch for 1 / 8 /
32 queries (NQS) of two kinds -- `selective`: two-term ANDs over the 200 most frequent terms, `broad`: the OR half of
C3's queries_bool5, five terms of the 1000 most frequent --, pages of 1 000 / 100 000 / NXS_MATCH_MAX ids (LIMITS), the first page (cursor 0) and a page from
mid-collection (cursor DOCS / 2; doc ids are 1..DOCS).  STEPS calls per cell give the HIP-event ms of k_md_mask,
k_md_from, k_md_count, k_md_scan and k_md_emit per call, the passes, the ids per call and the wall-clock ms of the C
call (median; the binding's conversion into Python lists is NOT in it: the objects are released unread).

Beside them, per kind and number of queries, the two things to set them against:
  floor   the count pass of the same plans -- "total" through k_count_tile (NXS_GPU_COUNT=tile), whose body the mask
          kernel is: HIP-event ms of the count kernels per batch.  `x_floor` = (mask + from + count + scan + emit) / floor.
  search  what a user does without the call: search_batch of the same queries at limit = min(the largest |M|,
          SEARCH_CAP = 100 000): wall-clock ms and the scans' + replays' HIP-event ms, ONE call each, first use of that
          limit included (run last; the record is saved after every step).
`runs` tries NXS_GPU_MATCHDOCS_RUN in 256 / 1024 / 4096 on the broad 32-query first page of 1 000.

These figures are a record, not a verdict.  Reads nothing but its own corpus.  Prints one JSON line; OUT=path writes
it there too (default profiles/matchdocs_probe.json), stamped with the source hash bench.py uses."""
import ctypes as C
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
STEPS = max(2, int(os.environ.get("STEPS", 3)))
NQS = [int(x) for x in os.environ.get("NQS", "1,8,32").split(",")]
MATCH_MAX = 1 << 22
LIMITS = [int(x) for x in os.environ.get("LIMITS", "1000,100000,%d" % MATCH_MAX).split(",")]
RUNS = [int(x) for x in os.environ.get("RUNS", "256,1024,4096").split(",")]
SEARCH_CAP = int(os.environ.get("SEARCH_CAP", 100_000))
work = os.environ.get("WORK", "/dev/shm/nxs_matchdocs_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "matchdocs_probe.json"))
KERNELS = ("mask", "from", "count", "scan", "emit")


def source_hash():
    """(= bench.py's)"""
    root = os.path.join(ROOT, "nxsearch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def call(idx, qs, limit, start):
    """one nxs_index_match_docs_batch through the C ABI -> (wall ms, counts, totals); the objects are released unread"""
    L = N.lib()
    n = len(qs)
    p = L.nxs_params_create()
    L.nxs_params_set_uint(p, b"match_limit", limit)
    L.nxs_params_set_uint(p, b"match_from", start)
    L.nxs_params_set_bool(p, b"fuzzymatch", False)
    out, errs = (C.c_void_p * n)(), (C.c_int * n)()
    arr = (C.c_char_p * n)(*[q.encode() for q in qs])
    t0 = time.perf_counter()
    r = L.nxs_index_match_docs_batch(idx._h, p, arr, n, None, out, errs)
    ms = 1e3 * (time.perf_counter() - t0)
    L.nxs_params_release(p)
    if r != 0:
        raise RuntimeError("match_docs failed: %r" % (idx.nxs.error(),))
    counts = [L.nxs_docs_count(out[i]) for i in range(n)]
    totals = [L.nxs_docs_total(out[i]) for i in range(n)]
    for i in range(n):
        L.nxs_docs_release(out[i])
    return ms, counts, totals


def timed(idx, qs, limit, start, steps=STEPS):
    call(idx, qs, limit, start)                             # (the workspace grows with the first call of a shape)
    idx.match_docs_profile(reset=True)
    wall = []
    for _ in range(steps):
        ms, counts, totals = call(idx, qs, limit, start)
        wall.append(ms)
    p = idx.match_docs_profile(reset=True)
    n = float(steps)
    r = {"wall_ms": round(statistics.median(wall), 3), "passes_per_call": p["passes"] / n, "ids_per_call": p["ids"] / n,
         "pairs_per_call": p["device_pairs"] / n}
    for k in KERNELS:
        r["k_md_%s_ms" % k] = round(p[k + "_ms"] / n, 4)
    r["kernels_ms"] = round(sum(p[k + "_ms"] for k in KERNELS) / n, 4)
    r["dominant"] = "k_md_" + max(KERNELS, key=lambda k: p[k + "_ms"])
    return r, totals


def save(res):
    """the record so far as one JSON line, written to OUT (a run that is cut short keeps what it has)"""
    line = json.dumps(res, sort_keys=True)
    if out_path:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")
    return line


def main():
    res = {"what": "match_docs: HIP-event ms of nxsgpu_match_docs' kernels per call (mean of %d calls) and wall-clock ms of "
                   "the C call (median) on C3, against the count pass of the same plans (floor) and a search at a large "
                   "limit" % STEPS,
           "source_hash": source_hash(), "docs": DOCS, "terms": TERMS, "steps": STEPS, "cells": {}, "floor": {}, "search": {}}
    os.makedirs(work, exist_ok=True)
    c = corpus.write_corpus(work, DOCS, TERMS, seed=0)
    terms = corpus.term_strings(TERMS, seed=0)
    nxs = N.Nxs(work)
    idx = nxs.open_files(c["terms"], c["dtmap"], algo="BM25")
    idx.set_plan_cache(False)
    res["postings"] = int(N.lib().nxsgpu_index_postings(idx.device))
    idx.set_profiling(True)
    nmax = max(NQS)
    text = lambda qs: [q.decode() if isinstance(q, bytes) else q for q in qs]
    kinds = {"selective": text(corpus.queries_bool5(terms, 2 * nmax, seed=22, hi=200, k=2))[0::2],
             "broad": text(corpus.queries_bool5(terms, 2 * nmax, seed=21, hi=1000))[1::2]}
    all_totals = {}
    for kind, qs_all in kinds.items():
        for nq in NQS:
            qs = qs_all[:nq]
            key = "%s_%d" % (kind, nq)
            totals = None
            for limit in LIMITS:
                for where, start in (("first", 0), ("mid", DOCS // 2)):
                    r, totals = timed(idx, qs, limit, start)
                    res["cells"]["%s_%d_%s" % (key, limit, where)] = r
                    print("[matchdocs_probe] %s limit %d %s: %s" % (key, limit, where, r), file=sys.stderr, flush=True)
            res["cells"][key + "_mean_total"] = round(sum(totals) / float(nq), 1)
            # (a) the floor: the count pass of the same plans through k_count_tile
            os.environ["NXS_GPU_COUNT"] = "tile"
            idx.reconfigure()
            idx.search_batch(qs, limit=10, fuzzymatch=False, total=True)
            idx.count_profile(reset=True)
            for _ in range(STEPS):
                idx.search_batch(qs, limit=10, fuzzymatch=False, total=True)
            p = idx.count_profile(reset=True)
            del os.environ["NXS_GPU_COUNT"]
            idx.reconfigure()
            floor = (p["tile"]["ms"] + p["req"]["ms"]) / STEPS
            res["floor"][key] = {"count_kernels_ms": round(floor, 4), "tile_queries": p["tile"]["queries"] / STEPS,
                                 "req_queries": p["req"]["queries"] / STEPS}
            for limit in LIMITS:
                for where in ("first", "mid"):
                    cell = res["cells"]["%s_%d_%s" % (key, limit, where)]
                    cell["x_floor"] = round(cell["kernels_ms"] / floor, 2) if floor > 0 else None
            all_totals[key] = totals
            save(res)
    # the run length, on the broad first page of 1 000 at the largest batch
    res["runs"] = {}
    for run in RUNS:
        os.environ["NXS_GPU_MATCHDOCS_RUN"] = str(run)
        idx.reconfigure()
        r, _ = timed(idx, kinds["broad"][:nmax], 1000, 0, steps=max(STEPS, 5))
        res["runs"][str(run)] = {k: r[k] for k in ("kernels_ms", "k_md_count_ms", "k_md_scan_ms", "k_md_emit_ms", "wall_ms")}
    del os.environ["NXS_GPU_MATCHDOCS_RUN"]
    idx.reconfigure()
    res["fastest_run"] = int(min(res["runs"], key=lambda k: res["runs"][k]["kernels_ms"]))
    save(res)
    # (b) what a user does today: a search at limit = min(the largest |M|, large); one call each, last: the slowest path
    for kind, qs_all in kinds.items():
        for nq in NQS:
            qs = qs_all[:nq]
            key = "%s_%d" % (kind, nq)
            k = max(1, min(max(all_totals[key]), SEARCH_CAP))
            idx.profile(reset=True)
            t0 = time.perf_counter()
            idx.search_batch(qs, limit=k, fuzzymatch=False)
            ms = 1e3 * (time.perf_counter() - t0)
            p = idx.profile(reset=True)
            res["search"][key] = {"limit": k, "wall_ms": round(ms, 3), "scan_ms": round(p["scan_ms"], 4),
                                  "replay_ms": round(p["replay_ms"], 4), "kernels_ms": round(p["scan_ms"] + p["replay_ms"], 4)}
            print("[matchdocs_probe] %s search %s" % (key, res["search"][key]), file=sys.stderr, flush=True)
            save(res)
    idx.set_profiling(False)
    idx.close()
    nxs.close()
    print(save(res))
    if not os.environ.get("KEEP"):
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
