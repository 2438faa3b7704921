#!/usr/bin/env python
"""Same-box A/B of builds on the slop phrase batches whose time per step is the host's enqueue (the plan of
sa_span_counts_batch runs on the clock of every run()):

  python scripts/slop_host_ab.py --libs build/libsearcharray_hip_parent.so,searcharray_amd/libsearcharray_hip.so --reps 7

Workloads on zipf-1M: the bench's `slop_batch` leg (256 two-token slop-2 phrases) and the batches of
scripts/slop_terms_batch_prof.py for 2 and 3 terms.  The libraries are loaded side by side in one process (ctypes,
RTLD_LOCAL), each builds its own index from the same corpus, and they ALTERNATE inside every repetition; the whole is
done once per order of building the indexes ("built": 0 = first).  One JSON line per (repetition, library, workload): ms
per step by the host clock over `--steps` asynchronous runs, the host's enqueue alone, kernel ms by HIP events, results
equal to the first library's; then one summary line per workload: every library's ms_per_step against the spread
(min .. max) of the FIRST library's own repetitions."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                        # noqa: E402
from searcharray_amd import _lib                                    # noqa: E402
from searcharray_amd.device_index import DeviceIndex                # noqa: E402


def terms_batch(T):
    """the recipe of scripts/slop_terms_batch_prof.py"""
    rng = np.random.default_rng(9)
    phrases = []
    for i in range(256):
        lo, hi = (49, 5000) if i % 2 == 0 else (0, 50)
        ph = []
        while len(ph) < T:
            x = int(rng.integers(lo, hi))
            if x not in ph:
                ph.append(x)
        phrases.append(ph)
    return phrases


def timed(index, batch, n_warm, n_steps):
    """ms per step (host clock, asynchronous runs, one synchronize at the end), of which the host's enqueue alone (until the
    last run() has returned), kernel ms by HIP events"""
    for _ in range(n_warm):
        batch.run(sync=False)
    index.synchronize()
    batch.profile()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        batch.run(sync=False)
    t1 = time.perf_counter()
    index.synchronize()
    dt = time.perf_counter() - t0
    return dt / n_steps * 1e3, (t1 - t0) / n_steps * 1e3, batch.profile()[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="searcharray_amd/libsearcharray_hip.so")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    libs = args.libs.split(",")
    apis = []
    for lib in libs:
        path = lib if os.path.isabs(lib) else os.path.join(ROOT, lib)
        apis.append(_lib.bind(ctypes.CDLL(path), path, allow_missing=True))
    side = bench.PhraseSide(apis[0], 1_000_000, 100_000)           # (the corpus and the bench's phrases; its index is not measured)
    workloads = [("slop_batch", side.slop2), ("terms2", terms_batch(2)), ("terms3", terms_batch(3))]
    ms, ref = {}, {}
    # Where an index lies in device memory moves the kernel time of the SAME code object by 1 - 3 %, more than a change of the
    # host plan could (profiles/slop_host_plan_ab_single_order.jsonl), so every library is measured in every position of the
    # build order: one phase per rotation of the list
    for phase in range(len(libs)):
        order = [(i + phase) % len(libs) for i in range(len(libs))]
        indexes = {li: DeviceIndex(side.words, side.term_off, side.doc_lens, api=apis[li]) for li in order}
        batches = {li: [indexes[li].phrase_batch(ph, k=10, slop=2) for _, ph in workloads] for li in order}
        for rep in range(args.reps):
            for pos, li in enumerate(order):
                for wi, (name, _) in enumerate(workloads):
                    dt, enq, kms = timed(indexes[li], batches[li][wi], args.warmup, args.steps)
                    res = batches[li][wi].fetch()
                    r0 = ref.setdefault(name, res)
                    same = bool(np.array_equal(r0[0], res[0]) and np.array_equal(r0[1], res[1]))
                    ms.setdefault((name, li), []).append((dt, enq))
                    print(json.dumps({"rep": rep, "lib": os.path.basename(libs[li]), "built": pos, "workload": name, "ms_per_step": round(dt, 4),
                                      "host_enqueue_ms": round(enq, 4), "kernel_ms": round(kms, 4), "same_results": same}), flush=True)
        for li in order:
            for b in batches[li]:
                b.close()
            indexes[li].close()
    for name, _ in workloads:
        base = [v[0] for v in ms[(name, 0)]]
        out = {"workload": name, "summary": True, "first_lib_spread_ms": [round(min(base), 4), round(max(base), 4)]}
        for li, lib in enumerate(libs):
            v = [x[0] for x in ms[(name, li)]]
            e = [x[1] for x in ms[(name, li)]]
            out[os.path.basename(lib)] = {"median_ms_per_step": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                                          "median_host_enqueue_ms": round(float(np.median(e)), 4),
                                          "median_not_above_first_lib_spread": bool(float(np.median(v)) <= max(base))}
        print(json.dumps(out), flush=True)
    side.close()


if __name__ == "__main__":
    main()
