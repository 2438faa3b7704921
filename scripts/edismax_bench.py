#!/usr/bin/env python
"""edismax over a two-field frame: combination on the device (Part 4 of the C ABI) vs with numpy on the
host (the reference's way, over the same GPU score() vectors); and the ranked query: edismax_search(k=10), which selects
on the device, vs edismax() followed by the numpy selection a caller had to write before, without and with a 10 % fq.
--from-tokens builds the two columns from the synthetic token stream directly (the index is encoded on the device, no Python
strings: what makes 10 M docs practical; the documents are the same); --no-host-leg skips the numpy COMBINATION leg (minutes at
10 M docs).  --out FILE appends the JSON line to FILE (profiles/edismax_topk.jsonl)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from searcharray_amd.solr import edismax, edismax_search
from edismax_frame import build_frame

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=500_000)
ap.add_argument("--reps", type=int, default=7, help="timed repetitions of the ranked legs (median reported)")
ap.add_argument("--out", default=None)
ap.add_argument("--from-tokens", action="store_true")
ap.add_argument("--no-host-leg", action="store_true")
args = ap.parse_args()
D = args.docs
frame = build_frame(D, args.from_tokens)
params = dict(q="t3 t40 t7", qf=["title^3", "body"], pf=["body"], pf2=["title", "body"], mm="2<75%", tie=0.2)
out = {"docs": D, "frame": "tokens" if args.from_tokens else "strings"}
res = {}
for route in ((True,) if args.no_host_leg else (True, False)):
    edismax(frame, use_device=route, **params)
    t0 = time.perf_counter()
    for _ in range(5):
        res[route], _ = edismax(frame, use_device=route, **params)
    out["device_ms" if route else "host_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 2)
if not args.no_host_leg:
    out["identical"] = bool(np.array_equal(res[True], res[False]))
out["matches"] = int((res[True] > 0).sum())


def ranked_host(mask, k=10):
    """the only way to the ranked answer without edismax_search: the dense vector, then numpy on one host core"""
    v, _ = edismax(frame, **params)
    keep = v > 0 if mask is None else (v > 0) & mask
    idx = np.flatnonzero(keep)
    order = idx[np.lexsort((idx, -v[idx]))[:k]]
    return v[order], order.astype(np.uint64), len(idx)


def median_ms(fn, reps):
    fn()                                                          # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        times.append((time.perf_counter() - t0) * 1e3)            # (both legs are synchronous: they return host arrays)
    return round(float(np.median(times)), 3), r


mask = np.random.default_rng(7).random(D) < 0.1
fq = frame["title"].array.doc_filter(mask)
same = True
for tag, m, f in (("", None, None), ("_fq10", mask, fq)):
    out["search_ms" + tag], hits = median_ms(lambda: edismax_search(frame, k=10, fq=f, **params), args.reps)
    out["edismax_numpy_ms" + tag], want = median_ms(lambda: ranked_host(m), args.reps)
    n = len(want[1])
    same = same and hits.found == want[2] and np.array_equal(hits.rows[:n], want[1]) and np.array_equal(hits.scores[:n], want[0]) \
        and bool(np.all(hits.rows[n:] == np.uint64(2**64 - 1)))
    out["found" + tag] = hits.found
fq.close()
out["ranked_identical"] = bool(same)
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
