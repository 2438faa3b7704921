#!/usr/bin/env python
"""What a document filter costs and saves on the two phrase workloads of bench.py (its PhraseSide): a resident zipf-1M index, 256
consecutive trigrams sampled from random docs (the tile kernel) and 256 two-token slop-2 phrases, half on ranks 50-5000, half on
ranks 1-50 (the span kernels); a step is one run of the resident batch, top-10.

  python scripts/phrase_filter_bench.py [--parent-lib PATH] [--out profiles/phrase_filter.jsonl]

Legs, per workload (each warmed; a leg's time is the median of `--regions` regions of `--steps` steps; one JSON line per leg):
  a        unfiltered, this build              b1 / b2  unfiltered, the PARENT build's library (--parent-lib, loaded twice side by
  c        full filter (every doc eligible)             side, all three alternating region by region in one process: the spread
  d        random 50 % / 10 % / 1 %                     between b1 and b2 is the margin a is judged by -- gate 1)
  e        a contiguous 10 % / 1 % range       (gate 2: e at 1 % against c)
  today    the path a caller has without this: dense score(phrase, slop=) to the host, mask, argpartition -- 32 phrases of the
           workload, random 10 % filter (gate 3: its rate against d at 10 %)
Every leg's results are compared with the oracle on a sample of phrases (`--check` per workload)."""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refimpl as O                                              # noqa: E402
from searcharray_amd import synth, _lib                                     # noqa: E402
from searcharray_amd.device_index import DeviceIndex                        # noqa: E402


def workloads(lens, terms, vocab):
    """bench.py's PhraseSide: (name, phrases, slop)"""
    trigrams = [[int(t) for t in p] for p in synth.phrase_queries_from_tokens(lens, terms, 256, 3, seed=77)]
    rng = np.random.default_rng(5)
    slop2 = []
    for i in range(256):
        lo, hi = (49, min(5000, vocab - 1)) if i % 2 == 0 else (0, min(50, vocab - 1))
        a, b = (int(x) for x in rng.integers(lo, hi, 2))
        slop2.append([a, b + 1 if a == b else b])
    return [("trigrams", trigrams, 0), ("slop2", slop2, 2)]


class Side:
    """one library's index of the corpus + one resident batch per workload"""

    def __init__(self, name, api, words, term_off, doc_lens, loads):
        self.name, self.api = name, api
        self.index = DeviceIndex(words, term_off, doc_lens, api=api)
        self.batches = {wl: self.index.phrase_batch(phrases, k=10, slop=slop) for wl, phrases, slop in loads}
        self.filtered = hasattr(api, "sa_phrase_batch_set_filter")          # (the parent build has none: its legs are unfiltered)

    def close(self):
        for b in self.batches.values():
            b.close()
        self.index.close()


class Leg:
    def __init__(self, side, wl, name, mask_name, mask, warm):
        self.side, self.batch, self.mask = side, side.batches[wl], mask
        if side.filtered:
            f = side.index.doc_filter(mask=mask) if mask is not None else None
            self.batch.set_doc_filter(f)
            if f is not None:
                f.close()
        self.meta = {"workload": wl, "leg": name, "lib": side.name, "k": 10, "filter": mask_name or "none",
                     "eligible_docs": int(mask.sum()) if mask is not None else side.index.n_docs, "docs": side.index.n_docs,
                     "phrases_per_step": self.batch.B}
        self.region(warm)

    def region(self, n):
        self.side.index.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.batch.run(sync=False)
        self.result = self.batch.fetch()
        self.side.index.synchronize()
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--check", type=int, default=4, help="phrases per workload compared with the oracle on every leg")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libsearcharray_hip.so (legs b1 / b2)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phrase_filter.jsonl"))
    args = ap.parse_args()
    D, V = args.docs, args.vocab
    t0 = time.time()
    lens, terms = synth.zipf_batch_tokens(0, D, V, fast=True)
    words, counts = synth.encode_batch(lens, terms, V)
    words, term_off = synth.concat_term_major([(words, counts)], V)
    doc_lens = lens.astype(np.float32)
    loads = workloads(lens, terms, V)
    print(f"corpus: {D} docs in {time.time() - t0:.0f}s", file=sys.stderr, flush=True)
    orc = O.OracleIndex(words, np.arange(V), term_off, doc_lens, D)
    # the sample: spread over the workload (the slop set alternates mid-frequency and frequent terms)
    sample = {wl: [int(i) for i in np.linspace(0, len(phrases) - 1, args.check).round()] for wl, phrases, _ in loads}
    dense = {wl: {i: orc.score(list(phrases[i]), slop=slop) for i in sample[wl]} for wl, phrases, slop in loads}
    print(f"oracle sample in {time.time() - t0:.0f}s", file=sys.stderr, flush=True)

    def parent_side(nm):
        # (a private copy per load: the loader hands out ONE mapping per path)
        tmp = os.path.join(tempfile.mkdtemp(), os.path.basename(args.parent_lib))
        shutil.copy(args.parent_lib, tmp)
        return Side(nm, _lib.bind(ctypes.CDLL(tmp), tmp, allow_missing=True), words, term_off, doc_lens, loads)
    # (this build's index is made BETWEEN the two parent loads: where an index lands in HBM is part of what the two loads differ by)
    parents = [parent_side("parent build, load 1")] if args.parent_lib else []
    new = Side("this build", _lib.api(), words, term_off, doc_lens, loads)
    if args.parent_lib:
        parents.append(parent_side("parent build, load 2"))
    rng = np.random.default_rng(5)
    masks = {"full": np.ones(D, dtype=bool)}
    for pct in (50, 10, 1):
        masks[f"random {pct}%"] = rng.random(D) < pct / 100.0
    for pct in (10, 1):
        m = np.zeros(D, dtype=bool)
        m[D // 3: D // 3 + D * pct // 100] = True
        masks[f"contiguous {pct}%"] = m
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def verify(leg):
        scores, docs = leg.result
        for i, d in dense[leg.meta["workload"]].items():
            dd = d.copy()
            if leg.mask is not None:
                dd[~leg.mask] = 0
            ws, wd = O.topk(dd, 10)
            n = int((ws > 0).sum())
            if not (np.array_equal(scores[i, :n], ws[:n]) and np.array_equal(docs[i, :n], wd[:n]) and not scores[i, n:].any()):
                return False
        return True

    def measure(legs):
        """the legs alternate region by region: same clocks, same thermal state for all of them"""
        times = [[] for _ in legs]
        for r in range(args.regions):
            for j in range(len(legs)):                          # (the order rotates: nobody is always first)
                i = (j + r) % len(legs)
                times[i].append(legs[i].region(args.steps))
        med = []
        for leg, ts in zip(legs, times):
            ms = sorted(1e3 * t / args.steps for t in ts)
            med.append(float(np.median(ms)))
            emit(dict(leg.meta, ms_per_step=round(med[-1], 4), ms_per_step_min=round(ms[0], 4), ms_per_step_max=round(ms[-1], 4),
                      phrases_per_s=round(leg.batch.B / (med[-1] / 1e3)), equals_oracle=verify(leg), regions=args.regions,
                      steps_per_region=args.steps))
        return med

    for wl, phrases, slop in loads:
        # gate 1: a against b1 / b2, alternating
        med = measure([Leg(new, wl, "a", None, None, args.warmup)] + [Leg(p, wl, f"b{i}", None, None, args.warmup) for i, p in enumerate(parents, 1)])
        if len(med) == 3:
            a, b1, b2 = med
            emit({"workload": wl, "gate": 1, "what": "unfiltered step of this build against two loads of the parent's library, interleaved",
                  "a_ms": round(a, 4), "b1_ms": round(b1, 4), "b2_ms": round(b2, 4), "parent_spread_ms": round(abs(b1 - b2), 4),
                  "a_minus_parent_mean_ms": round(a - (b1 + b2) / 2, 4), "within_parent_spread": bool(abs(a - (b1 + b2) / 2) <= abs(b1 - b2))})
        got = {}
        for tag, mn in (("c", "full"), ("d", "random 50%"), ("d", "random 10%"), ("d", "random 1%"), ("e", "contiguous 10%"), ("e", "contiguous 1%")):
            got[mn] = measure([Leg(new, wl, tag, mn, masks[mn], args.warmup)])[0]
        emit({"workload": wl, "gate": 2, "what": "contiguous 1 % against the full filter", "full_ms": round(got["full"], 4),
              "contiguous_1pct_ms": round(got["contiguous 1%"], 4), "faster": bool(got["contiguous 1%"] < got["full"])})
        new.batches[wl].set_doc_filter(None)
        # gate 3: the path a caller has today for the same question -- dense score() to the host, mask, argpartition
        mask = masks["random 10%"]
        qs = phrases[:32]
        new.index.synchronize()
        t1 = time.perf_counter()
        for ph in qs:
            total = new.index.bm25_phrase_dense(ph, slop=slop)
            total[~mask] = 0
            top = np.argpartition(-total, 10)[:10]
            top = top[np.lexsort((top, -total[top]))]
        dt = time.perf_counter() - t1
        today = len(qs) / dt
        batch_rate = len(phrases) / (got["random 10%"] / 1e3)
        emit({"workload": wl, "gate": 3, "leg": "today", "what": "dense score(phrase, slop=) to the host + mask + argpartition, 32 phrases, random 10% filter",
              "k": 10, "docs": D, "seconds": round(dt, 3), "phrases_per_s": round(today, 1), "filtered_batch_phrases_per_s": round(batch_rate),
              "ratio": round(batch_rate / today, 1)})
    out.close()
    for sd in [new] + parents:
        sd.close()


if __name__ == "__main__":
    main()
