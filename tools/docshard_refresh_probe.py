#!/usr/bin/env python3
"""N4 refresh in isolation: a C3-size collection (10M docs, 1M terms) in 4 doc shards on one GPU,
and what one nxs_docshard_refresh() costs in four cases -- nothing changed, one appended doc, one
removed doc (held by shard 0), one doc with a new term.  The files are modified in place like an
indexer process would (block first, header counters and data_len last), on a private copy.
Prints one JSON line; OUT=path writes it there too."""
import json
import os
import shutil
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nxsearch_amd as N
from nxsearch_amd import corpus

docs, nterms = int(os.environ.get("DOCS", 10_000_000)), int(os.environ.get("TERMS", 1_000_000))
n_shards = int(os.environ.get("SHARDS", 4))
work = os.environ.get("WORK", "/dev/shm/nxs_docshard_refresh_probe")
shutil.rmtree(work, ignore_errors=True)
info = corpus.write_corpus(work, docs, nterms, seed=0)
terms = corpus.term_strings(nterms, 0)
dpath, tpath = info["dtmap"], info["terms"]


def hdr(f):
    f.seek(8)
    return struct.unpack(">QQI", f.read(20))


def append_block(doc_id, pairs):
    with open(dpath, "r+b") as f:
        data_len, tokens, n = hdr(f)
        blk = struct.pack(">QII", doc_id, sum(c for _, c in pairs), len(pairs))
        blk += b"".join(struct.pack(">II", t, c) for t, c in sorted(pairs))
        f.seek(32 + data_len)
        f.write(blk)
        f.flush()
        f.seek(8)
        f.write(struct.pack(">QQI", data_len + len(blk), tokens + sum(c for _, c in pairs), n + 1))


def remove_first_doc():
    with open(dpath, "r+b") as f:
        data_len, tokens, n = hdr(f)
        f.seek(32)
        doc_id, doc_len, _ = struct.unpack(">QII", f.read(16))
        f.seek(32)
        f.write(struct.pack(">Q", 0))
        f.seek(32 + data_len)
        f.write(struct.pack(">QII", doc_id, 0, 0))
        f.flush()
        f.seek(8)
        f.write(struct.pack(">QQI", data_len + 16, tokens - doc_len, n - 1))
    return doc_id


def append_term(word):
    with open(tpath, "r+b") as f:
        f.seek(8)
        data_len = struct.unpack(">I", f.read(4))[0]
        blk = struct.pack(">H", len(word)) + word + b"\0"
        blk += b"\0" * (-len(blk) % 8) + struct.pack(">Q", 2)
        f.seek(16 + data_len)
        f.write(blk)
        f.flush()
        f.seek(8)
        f.write(struct.pack(">I", data_len + len(blk)))


out = {"docs": docs, "terms": nterms, "shards": n_shards}
with N.Nxs(work) as nxs:
    t0 = time.perf_counter()
    shards = [nxs.open_shard(tpath, dpath, s, n_shards) for s in range(n_shards)]
    q = [terms[99].decode()]
    nxs.docshard_search_batch(shards, q, limit=10, fuzzymatch=False)       # collection-wide df, once
    out["open_and_attach_s"] = round(time.perf_counter() - t0, 2)

    def timed():
        t = time.perf_counter()
        r = nxs.docshard_refresh(shards)
        return round(1e3 * (time.perf_counter() - t), 3), r

    ms = []
    for _ in range(5):
        m, r = timed()
        assert r is False
        ms.append(m)
    out["nothing_changed_ms"] = min(ms)
    new_id = docs + 10
    append_block(new_id, [(t, 1 + (t % 3)) for t in (5, 17, 100, 101, 2000, 7, 9, 11, 13)])
    out["append_1_doc_ms"], r = timed()
    assert r is True
    gone = remove_first_doc()
    out["remove_1_doc_ms"], r = timed()
    assert r is True
    word = b"zzqxjkvbnm"
    append_term(word)
    append_block(new_id + 5, [(nterms + 1, 2), (5, 1)])
    out["append_doc_with_new_term_ms"], r = timed()
    assert r is True
    got = nxs.docshard_search_batch(shards, [word.decode(), terms[4].decode()], limit=1000, fuzzymatch=False)
    out["new_term_found"] = [d for d, _ in got[0]] == [new_id + 5]
    out["removed_doc_gone"] = all(d != gone for d, _ in got[1])
    for s in shards:
        s.close()
line = json.dumps(out)
print(line)
if os.environ.get("OUT"):
    os.makedirs(os.path.dirname(os.path.abspath(os.environ["OUT"])), exist_ok=True)
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
shutil.rmtree(work, ignore_errors=True)
