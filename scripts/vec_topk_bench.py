#!/usr/bin/env python
"""The selection alone (sa_vec_topk) on a dense device vector of --n entries: wall time per call of DeviceVec.topk against the
copy it replaces (fetch() and the numpy selection on the host), without and with a random 10 % DocFilter, the passes it took,
and the rate sa_stream_probe reports for reading the same bytes once.  A constant vector gives the worst-case pass count.
Run under `rocprofv3 --kernel-trace --stats -- python scripts/vec_topk_bench.py --profile --only float64:gamma:none` for the
summed kernel time of ONE leg: --profile makes exactly --reps identical topk calls and nothing else on the vector (the kernel
statistics divided by --reps are one call; the first call's kernels run as long as the others'), --only DTYPE:VALUES:FILTER
keeps one leg (and builds no index when that leg has no filter).  --out FILE appends the JSON lines to FILE."""
import argparse, ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from searcharray_amd import _lib, synth
from searcharray_amd.device_index import DeviceIndex, DeviceVec

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10_000_000)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--profile", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--only", default=None, metavar="DTYPE:VALUES:FILTER", help="e.g. float64:gamma:tenth")
args = ap.parse_args()
api = _lib.api()
n, k = args.n, args.k
rng = np.random.default_rng(1)


def median_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 3), r


def host_select(vec, mask):
    v = vec.fetch()
    keep = v > 0 if mask is None else (v > 0) & mask
    idx = np.flatnonzero(keep)
    order = idx[np.lexsort((idx, -v[idx]))[:k]]
    return v[order], order.astype(np.uint64), len(idx)


g = ctypes.c_double(0)
api.call("sa_stream_probe", 1 << 30, 1, 5, ctypes.byref(g))
only = tuple(args.only.split(":")) if args.only else None
mask = rng.random(n) < 0.1
ix = fq = None
if only is None or only[2] == "tenth":
    lens, terms = synth.zipf_batch_tokens(0, n, 64, mean_len=2, fast=True)
    words, counts = synth.encode_batch(lens, terms, 64)
    words, term_off = synth.concat_term_major([(words, counts)], 64)
    ix = DeviceIndex(words, term_off, lens.astype(np.float32), api=api)
    fq = ix.doc_filter(mask=mask)
lines = []
for dtype in (np.float64, np.float32):
    scores = rng.gamma(2.0, 3.0, n).astype(dtype)
    scores[rng.random(n) < 0.3] = 0                                 # a query matches a part of the corpus
    for values, vname in ((scores, "gamma"), (np.full(n, 1.75, dtype), "constant")):
        if only and only[:2] != (dtype.__name__, vname):
            continue
        vec = DeviceVec(api, n, dtype == np.float64).store(values)
        for f, m, fname in ((None, None, "none"), (fq, mask, "tenth")):
            if (vname == "constant" and fname == "tenth") or (only and only[2] != fname):
                continue
            out = {"n": n, "k": k, "dtype": dtype.__name__, "values": vname, "filter": fname, "stream_probe_gbps": round(g.value, 1)}
            if args.profile:
                for _ in range(args.reps):
                    got = vec.topk(k, filter=f)
                out["profiled_calls"] = args.reps
            else:
                out["topk_ms"], got = median_ms(lambda: vec.topk(k, filter=f), args.reps)
            out["passes"] = vec.topk_passes()
            out["bytes_once"] = n * values.itemsize + (n // 8 if f is not None else 0)
            out["read_once_ms_at_probe_rate"] = round(out["bytes_once"] / (g.value * 1e9) * 1e3, 4)
            if not args.profile:
                out["fetch_numpy_ms"], want = median_ms(lambda: host_select(vec, m), 3)
                c = len(want[1])
                out["identical"] = bool(got[2] == want[2] and np.array_equal(got[1][:c], want[1]) and np.array_equal(got[0][:c], want[0]))
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
        vec.close()
if ix is not None:
    fq.close()
    ix.close()
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
