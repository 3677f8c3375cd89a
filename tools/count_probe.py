#!/usr/bin/env python3
"""What the total match count costs, and what the count kernels gain over the exact path's count pass.

On the C3 corpus and batch (10M docs / 1M terms, 1024 five-term AND / OR queries) and on C2 (1M docs /
100k terms, 1024 single-term queries) a batch is timed through nxs_index_search_batch_begin/_end with four
batches in flight (the C consumer bench.py uses: csrc/nxs_benchloop.c, no Python in the timed loop) under
  off    no "total"
  scan   "total" with NXS_GPU_COUNT=scan: the exact path's own count pass (MODE_COUNT) -- the only way to
         the same totals without the count kernels, and the baseline
  auto   "total" with NXS_GPU_COUNT=auto: k_count_req / the exact path's count pass / the host, by the query's shape
  tile   (OR half only) NXS_GPU_COUNT=tile: k_count_tile, which auto does not use until it wins here
C3 is also timed on its AND half (auto: all k_count_req) and its OR half alone, so that each kernel is
compared with `scan` on the queries it is, or would be, routed.  A figure = the MEAN ms per batch of one loop
of STEPS (>= 20) batches after a warm-up loop (the C loop has no clock per step: a step's own time is not
defined with four batches in flight); the loop is repeated REPEATS times per setting, settings interleaved;
reported: the median LOOP and the spread (max - min) of the repeated loops -- a median of loop means, not of
single steps.  How to read scan against auto: `scan` runs blocking inside _begin (the exact path's count pass
ends in a stream synchronisation on the host) while the count kernels are queued and overlap the batch's
scans, so the step-time margin holds both the kernels' work and the pipelining; the kernels alone are the
"kernels" record (HIP events) -- set that against count_ms_scan of the same set.  With profiling on
a further loop gives the HIP-event time of each count kernel alone.  Reads nothing but its own corpus.
Prints one JSON line; OUT=path writes it there too (default profiles/count_probe.json)."""
import ctypes as C
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

STEPS = max(20, int(os.environ.get("STEPS", 24)))
REPEATS = int(os.environ.get("REPEATS", 5))
SETS = 4
work = os.environ.get("WORK", "/dev/shm/nxs_count_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "count_probe.json"))


class BenchOut(C.Structure):
    _fields_ = [("seconds", C.c_double), ("results", C.c_uint64), ("checksum", C.c_uint64), ("failed", C.c_uint64)]


L = N.lib()
B = C.CDLL(os.path.join(N.CSRC, "libnxsbench.so"))
B.nxs_bench_batches_rot.restype = C.c_int
B.nxs_bench_batches_rot.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_size_t, C.c_uint,
                                    C.c_uint, C.c_int, C.POINTER(BenchOut)]


def loop(idx, params, arr, n, steps):
    o = BenchOut()
    if B.nxs_bench_batches_rot(idx._h, params, arr, n, SETS, steps, 4, C.byref(o)) != 0:
        raise RuntimeError("bench loop failed: %r" % (idx.nxs.error(),))
    assert o.failed == 0
    return 1e3 * o.seconds / steps, o.checksum


def measure(idx, name, sets, with_tile=False):
    """sets: SETS batches of equal size -> the record of one query set"""
    n = len(sets[0])
    arr = (C.c_char_p * (n * SETS))(*[q.encode() for b in sets for q in b])
    settings = {"off": (None, False), "scan": ("scan", True), "auto": ("auto", True)}
    if with_tile:
        settings["tile"] = ("tile", True)
    params = {k: N._make_params(limit=10, fuzzymatch=False, total=tot) for k, (_, tot) in settings.items()}
    ms = {k: [] for k in settings}
    sums = {}
    for rep in range(REPEATS + 1):
        for k, (mode, _) in settings.items():
            os.environ["NXS_GPU_COUNT"] = mode or "auto"
            idx.reconfigure()
            t, cs = loop(idx, params[k], arr, n, STEPS)
            sums.setdefault(k, cs)
            if rep:                                     # (rep 0: warm-up)
                ms[k].append(t)
    assert len(set(sums.values())) == 1, sums          # the same results with and without the total
    rec = {"queries_per_batch": n, "steps_per_loop": STEPS, "loops": REPEATS}
    for k in settings:
        med = statistics.median(ms[k])
        rec[k] = {"ms_per_batch": round(med, 4), "spread_ms": round(max(ms[k]) - min(ms[k]), 4),
                  "loops_ms": [round(x, 4) for x in ms[k]], "queries_per_s": round(1e3 * n / med)}
    rec["count_ms_scan"] = round(rec["scan"]["ms_per_batch"] - rec["off"]["ms_per_batch"], 4)
    rec["count_ms_auto"] = round(rec["auto"]["ms_per_batch"] - rec["off"]["ms_per_batch"], 4)
    spread = max(rec[k]["spread_ms"] for k in ("scan", "auto"))
    rec["auto_below_scan_by_ms"] = round(rec["scan"]["ms_per_batch"] - rec["auto"]["ms_per_batch"], 4)
    rec["margin_exceeds_spread"] = rec["auto_below_scan_by_ms"] > spread
    rec["total_on_costs_qps"] = rec["off"]["queries_per_s"] - rec["auto"]["queries_per_s"]
    # the count kernels alone (HIP events around them, on their own stream)
    os.environ["NXS_GPU_COUNT"] = "auto"
    idx.reconfigure()
    idx.set_profiling(True)
    os.environ["NXS_GPU_COUNT"] = "tile" if with_tile else "auto"
    idx.reconfigure()
    idx.count_profile(reset=True)
    loop(idx, params["auto"], arr, n, STEPS)
    p = idx.count_profile(reset=True)
    idx.set_profiling(False)
    rec["kernels"] = {k: {"launches": v["launches"], "queries_per_launch": v["queries"] / max(v["launches"], 1),
                          "ms_per_launch": round(v["ms"] / max(v["launches"], 1), 4)}
                      for k, v in (("k_count_tile", p["tile"]), ("k_count_req", p["req"]))}
    for pp in params.values():
        if pp:
            L.nxs_params_release(pp)
    print("[count_probe] %s: off %.3f  scan %.3f  auto %.3f ms/batch (spread %.3f)" % (
        name, rec["off"]["ms_per_batch"], rec["scan"]["ms_per_batch"], rec["auto"]["ms_per_batch"], spread),
        file=sys.stderr, flush=True)
    return rec


def main():
    out = {"tool": "tools/count_probe.py", "depth": 4, "limit": 10,
           "figure": "median over `loops` loops of the mean ms per batch of a loop of `steps_per_loop` batches",
           "note": "scan runs blocking inside _begin, the count kernels overlap the scans: the step-time margin holds "
                   "pipelining as well as kernel work; `kernels` is the count kernels' HIP-event time alone",
           "sets": {}}
    for wl, docs, nterms in (("C3", int(os.environ.get("C3_DOCS", 10_000_000)), int(os.environ.get("C3_TERMS", 1_000_000))),
                             ("C2", int(os.environ.get("C2_DOCS", 1_000_000)), int(os.environ.get("C2_TERMS", 100_000)))):
        d = os.path.join(work, wl)
        shutil.rmtree(d, ignore_errors=True)
        t0 = time.time()
        info = corpus.write_corpus(d, docs, nterms, seed=0)
        terms = corpus.term_strings(nterms, 0)
        print("[count_probe] %s corpus in %.0f s" % (wl, time.time() - t0), file=sys.stderr, flush=True)
        with N.Nxs(d) as nxs:
            idx = nxs.open_files(info["terms"], info["dtmap"])
            idx.set_plan_cache(False)
            if wl == "C3":
                full = [corpus.queries_bool5(terms, 1024, seed=3 + 100 * v, hi=1000) for v in range(SETS)]
                out["sets"]["C3"] = measure(idx, "C3", full)
                out["sets"]["C3_and_half"] = measure(idx, "C3 AND half", [b[0::2] for b in full])
                out["sets"]["C3_or_half"] = measure(idx, "C3 OR half", [b[1::2] for b in full], with_tile=True)
            else:
                out["sets"]["C2"] = measure(idx, "C2", [corpus.queries_single(terms, 1024, seed=3 + 100 * v) for v in range(SETS)])
            idx.close()
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
