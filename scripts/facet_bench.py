#!/usr/bin/env python
"""What hit counts and facet counts cost on the headline corpus: 10 M synthetic Zipf docs, 256 x 4-term BASELINE-shaped queries, a
column of 20 values (the LDS histogram) and one of 5000 (direct global atomics).

  python scripts/facet_bench.py [--out profiles/facets.jsonl]

Legs (all in one process, alternating round by round; a leg's time is the median of `--rounds` rounds of `--reps` synchronous calls;
one JSON line per leg):
  a/<state>/<column>   QueryBatch.facet_counts of the batch in <state> -- plain, m=2 (minimum-should-match 2 on every query), filter (a
                       random 10 % document filter) -- over <column>: V=20, V=5000, or found (codes == NULL, hit counts alone)
  b/<state>            run(sync=True) of a batch in the same state forced onto the per-query tile route (stage = 0, sparse = 0,
                       group = 0, k = 10): it reads the same postings, so it is the yardstick for the facet kernel
  c                    the host loop the call replaces, on the first `--sample` queries: a dense score per term to the host, the
                       same mm / filter logic again in numpy, np.bincount
Every a leg's counts are compared with c's on the sample (`parity`).  The summary line holds a / b for both columns."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from searcharray_amd import synth, _lib                                     # noqa: E402
from searcharray_amd.device_index import DeviceIndex                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "facets.jsonl"))
    args = ap.parse_args()
    D, V, B = args.docs, args.vocab, args.queries
    t0 = time.time()
    corpus = synth.zipf_corpus(D, vocab=V, workers=8)
    print(f"corpus: {D} docs in {time.time() - t0:.0f}s", file=sys.stderr, flush=True)
    queries = synth.bm25_queries(B, vocab=V)
    T = queries.shape[1]
    dev = DeviceIndex(corpus.words, corpus.term_off, corpus.doc_lens, tile_docs=args.tile, api=_lib.api())
    df = dev.docfreqs().astype(np.uint64)
    idf_table = np.log(1 + (D - df + 0.5) / (df + 0.5)).astype(np.float32)
    idf = idf_table[queries]
    info = dev.info()
    rng = np.random.default_rng(7)
    codes = {"V=20": (rng.integers(0, 20, D).astype(np.int32), 20), "V=5000": (rng.integers(0, 5000, D).astype(np.int32), 5000)}
    codes["V=20"][0][rng.random(D) < 0.05] = -1
    mask = rng.random(D) < 0.10
    cols = {name: dev.facet_column(c, nv) for name, (c, nv) in codes.items()}
    cols["found"] = None
    filt = dev.doc_filter(mask=mask)
    states = {"plain": {}, "m=2": {"min_match": [2] * B}, "filter": {"filter": filt}}
    tiles_only = {"stage": 0, "sparse": 0, "group": 0}
    a_bt = {s: dev.batch(queries, k=10, idf=idf, **kw) for s, kw in states.items()}
    b_bt = {s: dev.batch(queries, k=10, idf=idf, opts=tiles_only, **kw) for s, kw in states.items()}
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    # c: the host loop, timed on the sample; its counts are what every a leg is compared with
    S = min(args.sample, B)
    want, c_ms = {}, {}
    for state in states:
        t0 = time.perf_counter()
        rows = []
        for qi in range(S):
            per = [dev.bm25_dense([int(t)], idf=idf[qi, j:j + 1]) for j, t in enumerate(queries[qi])]
            dense = np.sum(per, axis=0)
            if state == "m=2":
                dense[np.sum([s > 0 for s in per], axis=0) < 2] = 0
            hit = dense > 0
            if state == "filter":
                hit &= mask
            rows.append({name: (int(hit.sum()), int((hit & (c < 0)).sum()), np.bincount(c[hit & (c >= 0)], minlength=nv))
                         for name, (c, nv) in codes.items()})
        c_ms[state] = 1e3 * (time.perf_counter() - t0) / S
        want[state] = rows
        emit({"leg": "c", "state": state, "what": "dense score per term to the host + numpy + bincount (both columns)", "docs": D, "queries": S,
              "ms_per_query": round(c_ms[state], 2), "queries_per_s": round(1e3 / c_ms[state], 1)})

    def parity(state, col, got):
        found, missing, counts = got
        ref = want[state]
        name = "V=20" if col == "found" else col
        ok = all(int(found[qi]) == ref[qi][name][0] for qi in range(S))
        if col != "found":
            ok = ok and all(int(missing[qi]) == ref[qi][col][1] and np.array_equal(counts[qi], ref[qi][col][2]) for qi in range(S))
        return bool(ok)

    legs = [("a", s, c) for s in states for c in cols] + [("b", s, None) for s in states]
    times = {leg: [] for leg in legs}
    par = {}

    # the timed a legs are the library call itself into buffers that exist (no first-touch page faults, no dtype conversion in numpy)
    api = dev.api
    h_found, h_missing = np.zeros(B, dtype=np.uint64), np.zeros(B, dtype=np.uint64)
    h_counts = {name: np.ones((B, nv), dtype=np.uint32) for name, (c, nv) in codes.items()}

    def call(leg):
        kind, state, col = leg
        if kind == "b":
            b_bt[state].run(sync=True)
        elif col == "found":
            api.call("sa_batch_facet_counts", a_bt[state]._h, None, _lib.p_u64(h_found), None, None)
        else:
            api.call("sa_batch_facet_counts", a_bt[state]._h, cols[col]._h, _lib.p_u64(h_found), _lib.p_u64(h_missing), _lib.p_u32(h_counts[col]))

    for leg in legs:                                             # warm-up (tables, first launches) and the parity of every a leg
        if leg[0] == "a":
            par[leg] = parity(leg[1], leg[2], a_bt[leg[1]].facet_counts(cols[leg[2]]))
        call(leg)
        call(leg)
    for r in range(args.rounds):
        for j in range(len(legs)):                               # (the order rotates: nobody is always first)
            leg = legs[(j + r) % len(legs)]
            t0 = time.perf_counter()
            for _ in range(args.reps):
                call(leg)
            times[leg].append(1e3 * (time.perf_counter() - t0) / args.reps)
    med = {leg: float(np.median(ts)) for leg, ts in times.items()}
    for leg in legs:
        kind, state, col = leg
        ts = sorted(times[leg])
        rec = {"leg": f"{kind}/{state}" + (f"/{col}" if col else ""), "docs": D, "queries": B, "terms": T, "tile_docs": int(info.tile_docs),
               "ms_per_call": round(med[leg], 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4), "queries_per_s": round(B / (med[leg] / 1e3)),
               "rounds": args.rounds, "reps": args.reps}
        if kind == "a":
            rec["parity"] = par[leg]
            rec["ratio_a_to_b"] = round(med[leg] / med[("b", state, None)], 3)
            rec["speedup_over_c_per_query"] = round(c_ms[state] / (med[leg] / B), 1)
        else:
            rec["route"] = b_bt[state].last_route()
        emit(rec)
    emit({"leg": "summary", "a_over_b_V20": round(med[("a", "plain", "V=20")] / med[("b", "plain", None)], 3),
          "a_over_b_V5000": round(med[("a", "plain", "V=5000")] / med[("b", "plain", None)], 3),
          "V5000_over_V20": round(med[("a", "plain", "V=5000")] / med[("a", "plain", "V=20")], 3),
          "all_parity": all(par.values())})
    out.close()
    for x in list(a_bt.values()) + list(b_bt.values()) + [c for c in cols.values() if c is not None] + [filt]:
        x.close()
    dev.close()


if __name__ == "__main__":
    main()
