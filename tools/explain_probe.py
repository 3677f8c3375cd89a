#!/usr/bin/env python3
"""What explanations cost: the same rotated C3 batches with and without "explain".

On the C3 corpus (10M docs / 1M terms; DOCS / TERMS override) ROTATE (4) seed-distinct batches of BATCH (1024)
five-term AND / OR queries run through the consumer loop bench.py times (libnxsbench.so, the public API only,
plan cache off as there), at limit 10 and at the default limit of 1000, each with and without the key: STEPS
steps per loop, LOOPS loops alternating the two settings, the median ms per step of each.  Then, with profiling
on, the explain pass alone: HIP-event ms of k_explain per pass and per (result, token) cell, cells, cells
present, chunks -- and the batch's own `_end` wait (host profile) beside it.

The comparison is the same batch without the key on the same build; for batches that do not ask, bench.py's C3
line is the yardstick.  Reads nothing but its own corpus.  Prints one JSON line; OUT=path writes it there too
(default profiles/explain_probe.json), stamped with the source hash bench.py uses."""
import ctypes as C
import hashlib
import json
import os
import shutil
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nxsearch_amd as N
from nxsearch_amd import corpus

DOCS = int(os.environ.get("DOCS", 10_000_000))
TERMS = int(os.environ.get("TERMS", 1_000_000))
BATCH = int(os.environ.get("BATCH", 1024))
ROTATE = max(1, int(os.environ.get("ROTATE", 4)))
STEPS = max(4, int(os.environ.get("STEPS", 40)))
STEPS_BIG = max(4, int(os.environ.get("STEPS_BIG", 12)))
LOOPS = max(3, int(os.environ.get("LOOPS", 5)))
work = os.environ.get("WORK", "/dev/shm/nxs_explain_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "explain_probe.json"))


class BenchOut(C.Structure):
    _fields_ = [("seconds", C.c_double), ("results", C.c_uint64), ("checksum", C.c_uint64), ("failed", C.c_uint64)]


def source_hash():
    """(= bench.py's)"""
    root = os.path.join(ROOT, "nxsearch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def main():
    res = {"what": "explain: median ms per step of %d rotated C3 batches of %d queries with and without the key "
                   "(%d loops each, alternating), and the pass alone (HIP events)" % (ROTATE, BATCH, LOOPS),
           "source_hash": source_hash(), "docs": DOCS, "terms": TERMS, "batch": BATCH}
    os.makedirs(work, exist_ok=True)
    c = corpus.write_corpus(work, DOCS, TERMS, seed=0)
    terms = corpus.term_strings(TERMS, seed=0)
    batches = [corpus.queries_bool5(terms, BATCH, seed=3 + 100 * v, hi=1000) for v in range(ROTATE)]
    flat = [q for b in batches for q in b]
    qarr = (C.c_char_p * len(flat))(*[q.encode() for q in flat])
    nxs = N.Nxs(work)
    idx = nxs.open_files(c["terms"], c["dtmap"], algo="BM25")
    idx.set_plan_cache(False)
    L = N.lib()
    B = C.CDLL(os.path.join(N.CSRC, "libnxsbench.so"))
    B.nxs_bench_batches_rot.restype = C.c_int
    B.nxs_bench_batches_rot.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_size_t, C.c_uint,
                                        C.c_uint, C.c_int, C.POINTER(BenchOut)]

    def loop(params, steps, depth):
        out = BenchOut()
        if B.nxs_bench_batches_rot(idx._h, params, qarr, BATCH, ROTATE, steps, depth, C.byref(out)) != 0:
            raise N.NxsError(*nxs.error())
        assert out.failed == 0
        return 1e3 * out.seconds / steps, out.results

    for limit, steps in ((10, STEPS), (1000, STEPS_BIG)):
        depth = 4 if limit > 64 else 3
        p_off = N._make_params(limit, "BM25", False)
        p_on = N._make_params(limit, "BM25", False, explain=True)
        loop(p_off, max(4, steps // 2), depth)
        loop(p_on, max(4, steps // 2), depth)
        ms = {"off": [], "on": []}
        results = 0
        for _ in range(LOOPS):
            ms["off"].append(loop(p_off, steps, depth)[0])
            t, results = loop(p_on, steps, depth)
            ms["on"].append(t)
        # the batch's own _end wait without the key, then the pass alone beside the same steps with it
        idx.host_profile()
        loop(p_off, steps, depth)
        hp_off = idx.host_profile()
        idx.set_profiling(True)
        loop(p_on, 4, depth)
        idx.explain_profile(reset=True)
        idx.host_profile()
        loop(p_on, steps, depth)
        ep, hp = idx.explain_profile(reset=True), idx.host_profile()
        idx.set_profiling(False)
        n = float(max(ep["passes"], 1))
        res["limit%d" % limit] = {
            "steps": steps, "results_per_step": results // steps,
            "ms_per_step_off": round(statistics.median(ms["off"]), 4), "ms_per_step_on": round(statistics.median(ms["on"]), 4),
            "ms_per_step_off_all": [round(x, 4) for x in ms["off"]], "ms_per_step_on_all": [round(x, 4) for x in ms["on"]],
            "passes": ep["passes"], "chunks": ep["chunks"], "cells_per_pass": int(ep["cells"] / n),
            "present_per_pass": int(ep["present"] / n), "k_explain_ms_per_pass": round(ep["ms"] / n, 4),
            "k_explain_ns_per_cell": round(1e6 * ep["ms"] / max(ep["cells"], 1), 3),
            # host profile, ms per batch: the _end call, its wait for the device, building the responses
            "off_end_ms": hp_off["end_ms"], "off_end_wait_ms": hp_off["wait_ms"], "off_resps_ms": hp_off["resps_ms"],
            "on_end_ms": hp["end_ms"], "on_end_wait_ms": hp["wait_ms"], "on_resps_ms": hp["resps_ms"]}
        L.nxs_params_release(p_off)
        L.nxs_params_release(p_on)
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
