#!/usr/bin/env python
"""A list of multi-field queries: the Python loop of edismax_search (what a caller had before) against edismax_search_batch (one
fields batch, csrc/sa_fields.hip), on the two-field frame of scripts/edismax_bench.py (scripts/edismax_frame.py).

Workload: 256 queries of 3 to 4 tokens drawn from synth.bm25_queries, qf=["title^3", "body"], mm="2<75%", tie=0.2, k=10, no pf*;
then the same inside a random 10 % fq.  Legs, alternating in one process, after a warm-up, median of --reps (at least 7):
  (a) loop_ms    edismax_search per query
  (b) batch_ms   edismax_search_batch, wall clock: host planning, upload, kernels, fetch
  (c) kernel_ms  the score and merge kernels of the batch alone, by HIP events (a FieldsBatch driven directly, same inputs)
`identical`: every field of all 256 results equal between (a) and (b).  `alg_bytes`: 8 x the postings of every (query, clause,
field) term -- what an exhaustive scorer cannot avoid reading; kernel_ms as bytes/s of it and as a share of the 8.0 TB/s HBM peak is
an ALGORITHMIC rate, not measured traffic.  --out FILE appends the JSON line (profiles/edismax_batch.jsonl)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from searcharray_amd import solr, synth
from searcharray_amd.solr import edismax_search, edismax_search_batch
from edismax_frame import VOCAB, build_frame

HBM_PEAK = 8.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=500_000)
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--out", default=None)
ap.add_argument("--from-tokens", action="store_true")
args = ap.parse_args()
D, B, reps = args.docs, args.queries, max(7, args.reps)
frame = build_frame(D, args.from_tokens)
ids = synth.bm25_queries(B, vocab=VOCAB, seed=42)
queries = [" ".join(f"t{t}" for t in row[:3 + (i & 1)]) for i, row in enumerate(ids)]
params = dict(qf=["title^3", "body"], mm="2<75%", tie=0.2, k=args.k)
out = {"docs": D, "queries": B, "frame": "tokens" if args.from_tokens else "strings", "reps": reps, "k": args.k}


def same(a, b):
    return a.found == b.found and a.explain == b.explain and a.scores.dtype == b.scores.dtype and \
        np.array_equal(a.rows, b.rows) and np.array_equal(a.scores, b.scores)


mask = np.random.default_rng(7).random(D) < 0.1
fq = frame["title"].array.doc_filter(mask)
identical = True
for tag, f in (("", None), ("_fq10", fq)):
    def loop():
        return [edismax_search(frame, q, fq=f, **params) for q in queries]

    def batch():
        return edismax_search_batch(frame, queries, fq=f, **params)

    want, got = loop(), batch()                                   # warm-up: impact streams, scratch, page-locked pools
    identical = identical and all(same(a, b) for a, b in zip(want, got))
    t_loop, t_batch = [], []
    for _ in range(reps):                                         # the legs alternate
        t0 = time.perf_counter(); loop(); t1 = time.perf_counter(); batch(); t2 = time.perf_counter()
        t_loop.append((t1 - t0) * 1e3); t_batch.append((t2 - t1) * 1e3)
    plans = [solr._plan(frame, q, params["qf"], params["mm"], None, None, None, "OR", solr.default_bm25) for q in queries]
    terms, weights, need = solr._fields_batch_inputs(plans, list(range(B)))
    fb = solr._fields_batch_open(plans[0].fields)
    fb.set_filter(f)
    fb.set_queries(terms, weights, need, k=params["k"], tie=params["tie"])
    fb.run()
    t_kernel = []
    for _ in range(reps):
        fb.run()
        t_kernel.append(fb.profile()[0])
    alg_bytes, slices = fb.profile()[1], fb.profile()[2]
    fb.close()
    out["loop_ms" + tag] = round(float(np.median(t_loop)), 2)
    out["loop_ms_spread" + tag] = [round(min(t_loop), 2), round(max(t_loop), 2)]
    out["batch_ms" + tag] = round(float(np.median(t_batch)), 3)
    out["batch_ms_spread" + tag] = [round(min(t_batch), 3), round(max(t_batch), 3)]
    out["speedup" + tag] = round(float(np.median(t_loop) / np.median(t_batch)), 1)
    out["kernel_ms" + tag] = round(float(np.median(t_kernel)), 4)
    out["alg_gbps" + tag] = round(alg_bytes / (float(np.median(t_kernel)) * 1e-3) / 1e9, 1)
    out["alg_share_of_hbm_peak" + tag] = round(alg_bytes / (float(np.median(t_kernel)) * 1e-3) / HBM_PEAK, 4)
    out["found_max" + tag] = int(max(h.found for h in got))
out["alg_bytes"] = int(alg_bytes)
out["slices"] = int(slices)
out["identical"] = bool(identical)
fq.close()
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
