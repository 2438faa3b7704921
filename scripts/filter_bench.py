#!/usr/bin/env python
"""What a document filter costs and saves on the headline workload (bench.py's shape): 10 M synthetic Zipf docs, 256 x 4-term
BASELINE-shaped queries, fresh rotating query sets stepped through a ring of batches (one sa_batch_step + fetch per step).

  python scripts/filter_bench.py [--parent-lib PATH] [--out profiles/filtered_batch.jsonl]

Legs (each warmed; a leg's time is the median of `--regions` regions of `--steps` steps; one JSON line per leg):
  a   unfiltered, this build                       b1 / b2  unfiltered, the PARENT build's library (--parent-lib, loaded twice
  c   full filter (every doc eligible)                      side by side, all three alternating region by region in one process:
  d   random 50 % / 10 % / 1 %                              the spread between b1 and b2 is the margin a is judged by)
  e   a contiguous 10 % / 1 % range                a0  unfiltered with term_seed = 0 (no starting bounds: what c is compared with)
  f   a, c and random 10 % again at k = 100
  today  the path a caller has without filters -- dense score() per term to the host, mask, sum, argpartition -- on 32 queries
Every leg's results are compared with the oracle on a sample of queries (`--check` per set 0)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refimpl as O                                              # noqa: E402
from searcharray_amd import synth, _lib                                     # noqa: E402
from searcharray_amd.device_index import DeviceIndex, QueryBatch            # noqa: E402


class Side:
    """one library's index of the corpus + a ring of batches per (k, options)"""

    def __init__(self, name, api, corpus, D, tile):
        self.name, self.api = name, api
        self.index = DeviceIndex(corpus.words, corpus.term_off, corpus.doc_lens, tile_docs=tile, api=api)
        df = self.index.docfreqs().astype(np.uint64)
        self.idf_table = np.log(1 + (D - df + 0.5) / (df + 0.5)).astype(np.float32)
        self.index.set_idf_table(self.idf_table)
        self.rings = {}

    def ring(self, sets, k, P, opts):
        key = (k, tuple(sorted(opts.items())))
        if key not in self.rings:
            self.rings[key] = [QueryBatch(self.index, sets[i % len(sets)], k=k, idf=self.idf_table[sets[i % len(sets)]], opts=opts) for i in range(P)]
        return self.rings[key]

    def close(self):
        for ring in self.rings.values():
            for b in ring:
                b.close()
        self.index.close()


class Stream:
    """the query stream of bench.py's main leg over one ring: step i hands batch i mod P the set i mod len(sets)"""

    def __init__(self, side, ring, sets):
        self.side, self.ring, self.sets = side, ring, [np.ascontiguousarray(q, dtype=np.uint32) for q in sets]
        self.pending = [None] * len(ring)
        self.results = {}
        self.i = 0

    def drain(self, b):
        if self.pending[b] is not None:
            self.results[self.pending[b]] = self.ring[b].fetch()
            self.pending[b] = None

    def steps(self, n):
        P = len(self.ring)
        for _ in range(n):
            b = self.i % P
            self.drain(b)
            si = self.i % len(self.sets)
            self.ring[b].step(self.sets[si])
            self.pending[b] = si
            self.i += 1
        for b in range(P):
            self.drain(b)
        self.side.index.synchronize()

    def region(self, n):
        self.side.index.synchronize()
        t0 = time.perf_counter()
        self.steps(n)
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--pipeline", type=int, default=6)
    ap.add_argument("--query-sets", type=int, default=8)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--check", type=int, default=4, help="queries of set 0 compared with the oracle per leg")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libsearcharray_hip.so (legs b1 / b2)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_batch.jsonl"))
    args = ap.parse_args()
    D, V, B = args.docs, args.vocab, args.queries
    t0 = time.time()
    corpus = synth.zipf_corpus(D, vocab=V, workers=8)
    print(f"corpus: {D} docs in {time.time() - t0:.0f}s", file=sys.stderr, flush=True)
    sets = [synth.bm25_queries(B, vocab=V) if i == 0 else synth.bm25_queries(B, vocab=V, seed=1000 + 131 * i) for i in range(max(2, args.query_sets))]
    orc = O.OracleIndex(corpus.words, np.arange(V), corpus.term_off, corpus.doc_lens, D)
    dense0 = [orc.score_terms_sum([int(t) for t in sets[0][qi]]) for qi in range(args.check)]
    def parent_side(nm):
        # (a private copy per load: the loader hands out ONE mapping per path)
        import shutil
        import tempfile
        tmp = os.path.join(tempfile.mkdtemp(), os.path.basename(args.parent_lib))
        shutil.copy(args.parent_lib, tmp)
        return Side(nm, _lib.bind(ctypes.CDLL(tmp), tmp, allow_missing=True), corpus, D, args.tile)
    # (this build's index is made BETWEEN the two parent loads: where an index lands in HBM is part of what the two loads differ by)
    sides = [parent_side("parent build, load 1")] if args.parent_lib else []
    new = Side("this build", _lib.api(), corpus, D, args.tile)
    sides = [new] + sides + ([parent_side("parent build, load 2")] if args.parent_lib else [])
    rng = np.random.default_rng(5)
    masks = {"full": np.ones(D, dtype=bool)}
    for pct in (50, 10, 1):
        masks[f"random {pct}%"] = rng.random(D) < pct / 100.0
    for pct in (10, 1):
        m = np.zeros(D, dtype=bool)
        m[D // 3: D // 3 + D * pct // 100] = True
        masks[f"contiguous {pct}%"] = m
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def verify(stream, mask, k):
        scores, docs = stream.results[0]
        for qi, d in enumerate(dense0):
            dd = d.copy()
            if mask is not None:
                dd[~mask] = 0
            ws, wd = O.topk(dd, k)
            n = int((ws > 0).sum())
            if not (np.array_equal(scores[qi, :n], ws[:n]) and np.array_equal(docs[qi, :n], wd[:n]) and not scores[qi, n:].any()):
                return False
        return True

    def leg(name, side, k, mask_name=None, opts=None):
        """a stream of `side` under the filter `mask_name`, warmed"""
        ring = side.ring(sets, k, args.pipeline, opts or {})
        f = side.index.doc_filter(mask=masks[mask_name]) if mask_name else None
        if f is not None or hasattr(side.api, "sa_batch_set_filter"):       # (the parent build has no filters: its legs are unfiltered)
            for b in ring:
                b.set_filter(f)
        s = Stream(side, ring, sets)
        s.steps(max(args.warmup, 2 * args.pipeline))
        s.meta = {"leg": name, "lib": side.name, "k": k, "filter": mask_name or "none", "eligible_docs": int(masks[mask_name].sum()) if mask_name else D,
                  "options": opts or {}, "docs": D, "queries_per_step": B}
        s.mask = masks[mask_name] if mask_name else None
        return s

    def measure(streams):
        """the streams alternate region by region: same clocks, same thermal state for all of them"""
        times = [[] for _ in streams]
        for r in range(args.regions):
            for j in range(len(streams)):                       # (the order rotates: nobody is always first)
                i = (j + r) % len(streams)
                times[i].append(streams[i].region(args.steps))
        for s, ts in zip(streams, times):
            ms = sorted(1e3 * t / args.steps for t in ts)
            emit(dict(s.meta, ms_per_step=round(float(np.median(ms)), 4), ms_per_step_min=round(ms[0], 4), ms_per_step_max=round(ms[-1], 4),
                      queries_per_s=round(B / (float(np.median(ms)) / 1e3)), route=s.ring[0].last_route(), group_info=s.ring[0].group_info(),
                      equals_oracle=verify(s, s.mask, s.meta["k"]), regions=args.regions, steps_per_region=args.steps))
        return [float(np.median(t)) for t in times]

    # gate 1: a against b1 / b2, alternating
    measure([leg("a", new, 10)] + [leg(f"b{i}", sd, 10) for i, sd in enumerate(sides[1:], 1)])
    measure([leg("a0", new, 10, opts={"term_seed": 0})])
    # c, d, e at k = 10 (one ring, the filter changed between legs)
    for tag, mn in (("c", "full"), ("d", "random 50%"), ("d", "random 10%"), ("d", "random 1%"), ("e", "contiguous 10%"), ("e", "contiguous 1%")):
        measure([leg(tag, new, 10, mn)])
    # the staged-tile route forced for a filtered set (the library's own rule: sa_stage_plan)
    for tag, mn in (("c/staged", "full"), ("d/staged", "random 10%"), ("e/staged", "contiguous 1%")):
        measure([leg(tag, new, 10, mn, opts={"stage": 1})])
    # f: k = 100
    for tag, mn in (("f/a", None), ("f/c", "full"), ("f/d", "random 10%")):
        measure([leg(tag, new, 100, mn)])
    # the path a caller has today for the same question: dense score() per term to the host, mask, sum, argpartition (32 queries, 10 % filter)
    mask = masks["random 10%"]
    qs = sets[0][:32]
    t0 = time.perf_counter()
    for q in qs:
        total = np.zeros(D, dtype=np.float32)
        for t in q:
            total += new.index.bm25_dense([int(t)])
        total[~mask] = 0
        top = np.argpartition(-total, 10)[:10]
        top = top[np.lexsort((top, -total[top]))]
    dt = time.perf_counter() - t0
    emit({"leg": "today", "what": "dense score() per term to the host + mask + sum + argpartition, 32 queries, random 10% filter", "k": 10, "docs": D,
          "seconds": round(dt, 3), "queries_per_s": round(len(qs) / dt, 1)})
    out.close()
    for sd in sides:
        sd.close()


if __name__ == "__main__":
    main()
