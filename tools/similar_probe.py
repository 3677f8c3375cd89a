#!/usr/bin/env python3
"""What a doc's term vector and a `similar` search cost.

On the C3 corpus (10M docs / 1M terms; DOCS / TERMS override) random live docs are the sources: with profiling
on, nxsgpu_doc_terms (through Index.doc_terms, mindf 2) for batches of 1, 64 and 1024 docs at k = 8 -- STEPS
calls per setting give the HIP-event ms of k_dv_ord, k_dv_scan and k_dv_merge per call, the wall-clock ms of the
call and the mean number of eligible terms --, the host route (NXS_GPU_DOCTERMS=host: the posting arrays copied
back, the same lookups on one host thread) beside it for the same docs, HOST_STEPS calls each (HOST=0 skips
it), and a `similar` batch of 1024 docs end to end at limit 10: wall-clock ms per call.

The host route copies d_doc_ids, d_post_dt and d_post[algo] back into pageable host memory on EVERY call (8 B a
doc, 16 B a posting: about 5 GB at the default C3 size, three times over in a run) and walks every list on one
thread: mind the box's free memory, or set HOST=0.

There is nothing to compare these figures with but the host route: they are a record, not a verdict.  Reads
nothing but its own corpus.  Prints one JSON line; OUT=path writes it there too (default
profiles/similar_probe.json), stamped with the source hash bench.py uses."""
import hashlib
import json
import os
import random
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
work = os.environ.get("WORK", "/dev/shm/nxs_similar_probe")
out_path = os.environ.get("OUT", os.path.join(ROOT, "profiles", "similar_probe.json"))


def source_hash():
    """(= bench.py's)"""
    root = os.path.join(ROOT, "nxsearch_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()[:16]


def timed(idx, docs, steps):
    """steps calls of Index.doc_terms -> (median wall ms, the profile per call, mean matches)"""
    idx.doc_terms_profile(reset=True)
    wall, got = [], None
    for _ in range(steps):
        t0 = time.perf_counter()
        got = idx.doc_terms(docs, limit=K, mindf=2)
        wall.append(1e3 * (time.perf_counter() - t0))
    p = idx.doc_terms_profile(reset=True)
    n = float(steps)
    return {"wall_ms": round(statistics.median(wall), 3), "k_dv_ord_ms": round(p["ord_ms"] / n, 4),
            "k_dv_scan_ms": round(p["scan_ms"] / n, 4), "k_dv_merge_ms": round(p["merge_ms"] / n, 4),
            "passes_per_call": p["passes"] / n, "calls": steps,
            "mean_matches": round(sum(g.matches for g in got) / float(len(got)), 1)}, got


def live_sources(idx, rng, n):
    """n random doc ids that are live docs (the synthetic corpus has ids 1 .. DOCS; one that is not would come
    back as an error slot)"""
    docs = [rng.randint(1, DOCS) for _ in range(n)]
    assert not any(isinstance(g, Exception) for g in idx.doc_terms(docs, limit=1)), "a source doc is not live"
    return docs


def main():
    res = {"what": "term vectors: HIP-event ms per call of nxsgpu_doc_terms at k = %d, mindf 2 (mean of %d calls), "
                   "wall-clock ms (median), the host route beside it; a similar batch end to end" % (K, STEPS),
           "source_hash": source_hash(), "docs": DOCS, "terms": TERMS, "k": K}
    os.makedirs(work, exist_ok=True)
    c = corpus.write_corpus(work, DOCS, TERMS, seed=0)
    rng = random.Random(11)
    nxs = N.Nxs(work)
    idx = nxs.open_files(c["terms"], c["dtmap"], algo="BM25")
    idx.set_profiling(True)
    idx.doc_terms([1], limit=K)         # (the pass's stream, events and workspace come with the first call)
    sources = {n: live_sources(idx, rng, n) for n in (1, 64, 1024)}
    device = {}
    for n, docs in sources.items():
        res["device_%d" % n], device[n] = timed(idx, docs, STEPS)
    if os.environ.get("HOST", "1") != "0":
        os.environ["NXS_GPU_DOCTERMS"] = "host"
        idx.reconfigure()
        for n, docs in sources.items():
            r, got = timed(idx, docs, HOST_STEPS)
            res["host_%d" % n] = {"wall_ms": r["wall_ms"], "calls": HOST_STEPS, "equal": got == device[n]}
        del os.environ["NXS_GPU_DOCTERMS"]
        idx.reconfigure()
    else:
        res["host"] = "not run"
    wall = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        got = idx.similar(sources[1024], limit=10, terms=K)
        wall.append(1e3 * (time.perf_counter() - t0))
    p = idx.doc_terms_profile(reset=True)
    res["similar_1024"] = {"wall_ms": round(statistics.median(wall), 3), "limit": 10,
                           "doc_terms_ms_per_call": round((p["ord_ms"] + p["scan_ms"] + p["merge_ms"]) / STEPS, 4),
                           "mean_results": round(sum(len(g) for g in got if not isinstance(g, Exception)) / float(len(got)), 2)}
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
