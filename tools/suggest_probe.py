#!/usr/bin/env python3
"""What spelling suggestions cost beside the fuzzy winner pass they share a screen with.

On the C4 corpus (10M docs / 1M terms; DOCS / TERMS override) and C4's own tokens (1024 existing terms with
one byte substituted, corpus.queries_fuzzy) the same process times, on the same tokens,
  fuzzy        Index.fuzzy(tokens): the match-first winner pass (nxsgpu_fuzzy)
  suggest k=5  Index.suggest(tokens, limit=5)
  suggest k=32 Index.suggest(tokens, limit=32)
each as wall-clock ms per call: after a warm-up loop (the first suggest call also builds the candidate
permutation: timed apart, as "candidate_build_ms"), REPEATS loops of STEPS calls, settings interleaved; a
figure = the median over the loops of the loop's mean, with the spread (max - min) of the loops.  The
yardstick is the fuzzy pass of this very run: the suggest pass runs the same screen over a candidate set
of its own and adds the distance of every survivor, the scatter and the selection.  With profiling on, a further
loop gives the HIP-event time of each part of both passes (nxsgpu_get_profile's fuzzy_* times,
nxsgpu_suggest_profile).  Reads nothing but its own corpus.  Prints one JSON line; OUT=path writes it there
too (default profiles/suggest_probe.json), stamped with the source hash bench.py uses."""
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
TOKENS = int(os.environ.get("TOKENS", 1024))
STEPS = max(5, int(os.environ.get("STEPS", 20)))
REPEATS = max(3, int(os.environ.get("REPEATS", 5)))
work = os.environ.get("WORK", "/dev/shm/nxs_suggest_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "suggest_probe.json"))


def source_hash():
    """(= bench.py's)"""
    root = os.path.join(ROOT, "nxsearch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def loop_ms(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    os.makedirs(work, exist_ok=True)
    c = corpus.write_corpus(work, DOCS, TERMS, seed=7)
    terms = corpus.term_strings(TERMS, seed=7)
    toks = [t if isinstance(t, bytes) else t.encode() for t in corpus.queries_fuzzy(terms, TOKENS, seed=4)]
    nxs = N.Nxs(work)
    idx = nxs.open_files(c["terms"], c["dtmap"])
    settings = {"fuzzy": lambda: idx.fuzzy(toks),
                "suggest_k5": lambda: idx.suggest(toks, limit=5),
                "suggest_k32": lambda: idx.suggest(toks, limit=32)}
    idx.fuzzy(toks)
    t0 = time.perf_counter()
    first = idx.suggest(toks, limit=5)
    first_ms = 1e3 * (time.perf_counter() - t0)
    for fn in settings.values():            # warm-up
        loop_ms(fn, 3)
    loops = {k: [] for k in settings}
    for _ in range(REPEATS):
        for k, fn in settings.items():
            loops[k].append(loop_ms(fn, STEPS))
    res = {"what": "C4: %d misspelt tokens over a %d-term dictionary; wall-clock ms per call through the Python "
                   "binding, median of %d loops of %d calls" % (len(toks), TERMS, REPEATS, STEPS),
           "source_hash": source_hash(), "docs": DOCS, "terms": TERMS, "tokens": len(toks)}
    for k, v in loops.items():
        res[k] = {"ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4),
                  "tokens_per_s": round(len(toks) / (statistics.median(v) * 1e-3), 1)}
    res["candidate_build_ms"] = round(first_ms - res["suggest_k5"]["ms"], 3)
    res["suggest_k5_over_fuzzy"] = round(res["suggest_k5"]["ms"] / res["fuzzy"]["ms"], 3)
    res["suggest_k32_over_fuzzy"] = round(res["suggest_k32"]["ms"] / res["fuzzy"]["ms"], 3)
    res["mean_matches"] = round(sum(s.matches for s in first) / float(len(first)), 2)
    # per kernel, HIP events
    idx.set_profiling(True)
    idx.suggest(toks[:8], limit=5)          # (the pass's events are created by the first profiled call)
    for k, lim in (("suggest_k5", 5), ("suggest_k32", 32)):
        idx.suggest_profile(reset=True)
        for _ in range(STEPS):
            idx.suggest(toks, limit=lim)
        p = idx.suggest_profile(reset=True)
        n = float(max(p["passes"], 1))
        res[k]["kernels"] = {"passes_per_call": p["passes"] / float(STEPS), "device_ms": round(p["ms"] / n, 4),
                             "peq_filter_ms": round(p["screen_ms"] / n, 4), "k_sg_dist_ms": round(p["dist_ms"] / n, 4),
                             "scan_scatter_ms": round(p["group_ms"] / n, 4), "k_sg_select_ms": round(p["select_ms"] / n, 4),
                             "survivors": int(p["survivors"] / n), "matches": int(p["matches"] / n),
                             "overflow_reruns": p["overflow_reruns"], "host_tokens": p["host_tokens"]}
    idx.profile(reset=True)
    for _ in range(STEPS):
        idx.fuzzy(toks)
    pr = idx.profile(reset=True)
    res["fuzzy"]["kernels"] = {"device_ms": round(pr["fuzzy_ms"] / STEPS, 4),
                               "peq_seed_filter_ms": round(pr["fuzzy_filter_ms"] / STEPS, 4),
                               "k_fz_dist_ms": round(pr["fuzzy_dist_ms"] / STEPS, 4),
                               "chain_finish_ms": round(pr["fuzzy_chain_ms"] / STEPS, 4),
                               "survivors": int(pr["fuzzy_level"][1] / STEPS)}
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
