#!/usr/bin/env python3
"""What prefix completion costs: the pass per kernel, and the build of the term order.

On the C4 dictionary (10M docs / 1M terms; DOCS / TERMS override) the first 1 / 2 / 3 / 5 bytes of C4's own
tokens (corpus.queries_fuzzy) are the prefixes, PREFIXES (1024) per pass, k = 5 and 32: with profiling on,
STEPS passes per setting give the HIP-event ms of k_px_range and k_px_select and of the pass (events around
both), and the mean range length (`matches`).  The first call builds the order: its wall-clock ms and
entries are reported apart (nxsgpu_complete_profile's build_ms).  Then, unless C5=0, the same build on the C5
dictionary (DOCS5 / TERMS5: 50M docs / 2M terms) -- one completion call on a fresh index.

There is nothing to compare these figures with: they are a record, not a verdict.  Reads nothing but its own
corpora.  Prints one JSON line; OUT=path writes it there too (default profiles/complete_probe.json), stamped
with the source hash bench.py uses."""
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
DOCS5 = int(os.environ.get("DOCS5", 50_000_000))
TERMS5 = int(os.environ.get("TERMS5", 2_000_000))
PREFIXES = int(os.environ.get("PREFIXES", 1024))
STEPS = max(3, int(os.environ.get("STEPS", 10)))
work = os.environ.get("WORK", "/dev/shm/nxs_complete_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "complete_probe.json"))


def source_hash():
    """(= bench.py's)"""
    root = os.path.join(ROOT, "nxsearch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def first_call(idx, prefixes):
    """the call that builds the order -> (wall ms of the call, the profile's build figures)"""
    t0 = time.perf_counter()
    idx.complete(prefixes, limit=5)
    ms = 1e3 * (time.perf_counter() - t0)
    p = idx.complete_profile()
    return {"first_call_ms": round(ms, 3), "build_ms": round(p["build_ms"], 3), "entries": p["entries"], "builds": p["builds"]}


def main():
    res = {"what": "prefix completion: HIP-event ms per pass of %d prefixes (mean of %d passes), wall-clock ms of the "
                   "order build" % (PREFIXES, STEPS), "source_hash": source_hash(), "prefixes": PREFIXES}
    d4 = os.path.join(work, "c4")
    os.makedirs(d4, exist_ok=True)
    c = corpus.write_corpus(d4, DOCS, TERMS, seed=7)
    terms = corpus.term_strings(TERMS, seed=7)
    toks = [t if isinstance(t, bytes) else t.encode() for t in corpus.queries_fuzzy(terms, PREFIXES, seed=4)]
    nxs = N.Nxs(d4)
    idx = nxs.open_files(c["terms"], c["dtmap"])
    res["c4"] = {"docs": DOCS, "terms": TERMS, "order": first_call(idx, [toks[0][:2]])}
    idx.set_profiling(True)
    idx.complete([toks[0][:1]], limit=5)        # (the pass's events are created by the first profiled call)
    for nb in (1, 2, 3, 5):
        px = [t[:nb] for t in toks]
        for k in (5, 32):
            idx.complete_profile(reset=True)
            got = None
            for _ in range(STEPS):
                got = idx.complete(px, limit=k)
            p = idx.complete_profile(reset=True)
            n = float(max(p["passes"], 1))
            res["c4"]["bytes%d_k%d" % (nb, k)] = {
                "pass_ms": round(p["ms"] / n, 4), "k_px_range_ms": round(p["range_ms"] / n, 4),
                "k_px_select_ms": round(p["select_ms"] / n, 4), "passes": p["passes"],
                "mean_matches": round(sum(g.matches for g in got) / float(len(got)), 1),
                "max_matches": max(g.matches for g in got)}
    idx.set_profiling(False)
    idx.close()
    nxs.close()
    if not os.environ.get("KEEP"):
        shutil.rmtree(d4, ignore_errors=True)
    if os.environ.get("C5", "1") != "0":
        d5 = os.path.join(work, "c5")
        os.makedirs(d5, exist_ok=True)
        c = corpus.write_corpus(d5, DOCS5, TERMS5, seed=7)
        nxs = N.Nxs(d5)
        idx = nxs.open_files(c["terms"], c["dtmap"])
        res["c5"] = {"docs": DOCS5, "terms": TERMS5, "order": first_call(idx, [toks[0][:2]])}
        idx.close()
        nxs.close()
        if not os.environ.get("KEEP"):
            shutil.rmtree(d5, ignore_errors=True)
    else:
        res["c5"] = "not run"
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
