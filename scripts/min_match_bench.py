#!/usr/bin/env python
"""What minimum-should-match and occur classes (+tok / -tok) cost and save on the headline workload (bench.py's shape): 10 M synthetic Zipf docs, 256 x 4-term
BASELINE-shaped queries at k = 10, fresh rotating query sets stepped through a ring of batches (one sa_batch_step + fetch per step).

  python scripts/min_match_bench.py [--parent-lib PATH] [--out profiles/min_match.jsonl]

Legs (each warmed; a leg's time is the median of `--regions` regions of `--steps` steps; one JSON line per leg):
  a/m=1, a/m=2, a/m=4   the batch with every value m, default options (values <= 1: the route of a batch without values)
  a/count               one query at 2, the others at 1: the counting kernels on all the work of b, nothing skipped but by that one query
  b                     no values, options stage = 0, sparse = 0, group = 0: the per-query tile route that the a legs with m > 1 take;
  b0                    b with term_seed = 0: without the starting bounds, which a batch with values > 1 never has
  b1 / b2               b on the PARENT build's library (--parent-lib, loaded twice side by side; b, b1 and b2 alternate region by
                        region in one process: the spread between b1 and b2 is the margin b is judged by -- a larger gap would mean
                        that the compile-time switch leaked into the old instantiations)
  skipped               share of the (tile, query) items the popcount shortcut left before reading a posting (sa_batch_stats)
  o/-t0, o/+t0, o/+t0-t1  occur classes on every query (sa_batch_set_occur), default options: slot 0 prohibited; slot 0 required; slot 0
                        required and slot 1 prohibited -- each beside p/plain and p/m=2, the PARENT build's plain batch (default
                        options) and its minimum-should-match batch (--parent-lib; without it this build's, marked so), alternating
                        region by region in one process
  c                     what a caller had before: edismax_search per query over a one-column frame of the same documents with the
                        same mm (`--edismax-queries` queries; the rows it returns must be those of leg a)
Every a / b leg's results are compared with the oracle on `--check` queries of set 0."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from filter_bench import Side, Stream                                       # noqa: E402
from oracle import refimpl as O                                              # noqa: E402
from searcharray_amd import synth, _lib                                     # noqa: E402
from searcharray_amd.device_index import QueryBatch                         # noqa: E402


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
    ap.add_argument("--edismax-queries", type=int, default=8, help="queries of set 0 for leg c (0: skip the leg)")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libsearcharray_hip.so (legs b1 / b2)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "min_match.jsonl"))
    args = ap.parse_args()
    D, V, B, K = args.docs, args.vocab, args.queries, 10
    t0 = time.time()
    corpus = synth.zipf_corpus(D, vocab=V, workers=8)
    print(f"corpus: {D} docs in {time.time() - t0:.0f}s", file=sys.stderr, flush=True)
    sets = [synth.bm25_queries(B, vocab=V) if i == 0 else synth.bm25_queries(B, vocab=V, seed=1000 + 131 * i) for i in range(max(2, args.query_sets))]
    orc = O.OracleIndex(corpus.words, np.arange(V), corpus.term_off, corpus.doc_lens, D)
    per0 = [[orc.score(int(t)) for t in sets[0][qi]] for qi in range(args.check)]

    def parent_side(nm):
        # (a private copy per load: the loader hands out ONE mapping per path)
        import ctypes
        import shutil
        import tempfile
        tmp = os.path.join(tempfile.mkdtemp(), os.path.basename(args.parent_lib))
        shutil.copy(args.parent_lib, tmp)
        return Side(nm, _lib.bind(ctypes.CDLL(tmp), tmp, allow_missing=True), corpus, D, args.tile)
    sides = [parent_side("parent build, load 1")] if args.parent_lib else []
    new = Side("this build", _lib.api(), corpus, D, args.tile)
    sides = [new] + sides + ([parent_side("parent build, load 2")] if args.parent_lib else [])
    info = new.index.info()
    out = open(args.out, "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    def verify(stream, values, occur=None):
        scores, docs = stream.results[0]
        for qi, per in enumerate(per0):
            m = 0 if values is None else int(values[qi])
            if occur is None:
                dense = np.sum(per, axis=0)
                if m > 1:
                    dense[np.sum([s > 0 for s in per], axis=0) < m] = 0
            else:                                                # (0 should, 1 must, 2 must_not; m counts the should slots)
                cl = [int(c) for c in occur[qi]]
                dense = np.sum([np.zeros_like(s) if c == 2 else s for s, c in zip(per, cl)], axis=0)
                ok = np.sum([s > 0 for s, c in zip(per, cl) if c == 0] or [np.zeros(D, dtype=bool)], axis=0) >= m
                for s, c in zip(per, cl):
                    ok &= (s > 0) if c == 1 else ~(s > 0) if c == 2 else True
                dense[~ok] = 0
            ws, wd = O.topk(dense, K)
            n = int((ws > 0).sum())
            if not (np.array_equal(scores[qi, :n], ws[:n]) and np.array_equal(docs[qi, :n], wd[:n]) and not scores[qi, n:].any()):
                return False
        return True

    def leg(name, side, values=None, opts=None, occur=None):
        # a ring of its own per leg (Side.ring shares rings by options): no leg depends on the values another one left behind
        ring = [QueryBatch(side.index, sets[i % len(sets)], k=K, idf=side.idf_table[sets[i % len(sets)]], opts=opts or {}) for i in range(args.pipeline)]
        side.rings[(name, side.name)] = ring                     # (closed with the side)
        if values is not None:
            for b in ring:
                b.set_min_match(values)
        if occur is not None:                                    # (only legs of this build carry classes: the parent has no such call)
            for b in ring:
                b.set_occur(occur)
        s = Stream(side, ring, sets)
        s.steps(max(args.warmup, 2 * args.pipeline))
        s.values, s.occur = values, occur
        s.meta = {"leg": name, "lib": side.name, "k": K, "min_match": "none" if values is None else sorted(set(int(v) for v in values)),
                  "occur": "none" if occur is None else "".join("s+-"[int(c)] for c in occur[0]), "options": opts or {}, "docs": D, "queries_per_step": B, "tile_docs": int(info.tile_docs)}
        return s

    def measure(streams):
        """the streams alternate region by region: same clocks, same thermal state for all of them"""
        times = [[] for _ in streams]
        for r in range(args.regions):
            for j in range(len(streams)):                       # (the order rotates: nobody is always first)
                i = (j + r) % len(streams)
                times[i].append(streams[i].region(args.steps))
        med = []
        for s, ts in zip(streams, times):
            ms = sorted(1e3 * t / args.steps for t in ts)
            med.append(float(np.median(ms)))
            emit(dict(s.meta, ms_per_step=round(med[-1], 4), ms_per_step_min=round(ms[0], 4), ms_per_step_max=round(ms[-1], 4),
                      queries_per_s=round(B / (med[-1] / 1e3)), route=s.ring[0].last_route(), seeds=bool(s.ring[0].seeds().any()),
                      equals_oracle=verify(s, s.values, s.occur), regions=args.regions, steps_per_region=args.steps))
        return med

    tiles_only = {"stage": 0, "sparse": 0, "group": 0}
    # b against b1 / b2, alternating: did the switch leak into the old instantiations?
    b_ms = measure([leg("b", new, None, tiles_only)] + [leg(f"b{i}", sd, None, tiles_only) for i, sd in enumerate(sides[1:], 1)])[0]
    # (b starts from the rank-table bounds, which a batch with values > 1 must do without: the same route with term_seed = 0)
    b0_ms = measure([leg("b0", new, None, dict(tiles_only, term_seed=0))])[0]
    # a: through the public API, default options
    one_two = np.ones(B, dtype=np.int64)
    one_two[0] = 2
    a_ms = {}
    for name, values in (("a/m=1", [1] * B), ("a/m=2", [2] * B), ("a/m=4", [4] * B), ("a/count", one_two)):
        a_ms[name] = measure([leg(name, new, values)])[0]
        emit({"leg": name, "ratio_a_to_b": round(a_ms[name] / b_ms, 3), "ratio_a_to_b0": round(a_ms[name] / b0_ms, 3)})
    # the popcount shortcut: (tile, query) items left before a posting was read, one run of set 0
    for m in (2, 4):
        bt = new.index.batch(sets[0], k=K, min_match=[m] * B)
        bt.stats(True)
        bt.run()
        skipped, _ = bt.stats(False)
        emit({"leg": "skipped", "min_match": m, "items": int(info.n_tiles) * B, "skipped": int(skipped), "share": round(skipped / (int(info.n_tiles) * B), 4)})
        bt.close()
    # occur classes: each pattern beside the parent build's plain and minimum-should-match batches
    base = sides[1] if args.parent_lib else new
    base_name = "" if args.parent_lib else " (THIS build: no --parent-lib)"
    T = sets[0].shape[1]
    for name, cls in (("o/-t0", [2] + [0] * (T - 1)), ("o/+t0", [1] + [0] * (T - 1)), ("o/+t0-t1", [1, 2] + [0] * (T - 2))):
        occ = np.tile(np.asarray(cls, dtype=np.uint8), (B, 1))
        o_ms, p_ms, pm_ms = measure([leg(name, new, None, None, occ), leg(f"p/plain beside {name}{base_name}", base), leg(f"p/m=2 beside {name}{base_name}", base, [2] * B)])
        emit({"leg": name, "ratio_to_parent_plain": round(o_ms / p_ms, 3), "ratio_to_parent_m2": round(o_ms / pm_ms, 3)})
    # c: edismax_search per query over a one-column frame of the same documents
    if args.edismax_queries:
        import pandas as pd
        from searcharray_amd import SearchArray
        from searcharray_amd.indexing import HostIndex
        from searcharray_amd.postings import _IndexCore, ws_tokenizer
        from searcharray_amd.solr import edismax_search
        from searcharray_amd.term_dict import TermDict
        batch_docs = 1_000_000                                   # (synth.zipf_corpus: the corpus is these seeded batches back to back)
        parts = [synth.zipf_batch_tokens(b, min(batch_docs, D - b * batch_docs), V, fast=True) for b in range((D + batch_docs - 1) // batch_docs)]
        lens = np.concatenate([p[0] for p in parts])
        terms = np.concatenate([p[1] for p in parts])
        del parts
        names = np.array([f"t{i}" for i in range(V)])
        present = np.unique(terms)
        term_dict = TermDict()
        term_dict.add_terms([str(t) for t in names[present]])
        remap = np.zeros(V, dtype=np.uint32)
        remap[present] = np.arange(len(present), dtype=np.uint32)
        host = HostIndex(term_dict, lens.astype(np.float32), tokens=np.ascontiguousarray(remap[terms]),
                         doc_ptr=np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens)]), dtype=np.uint64))
        arr = SearchArray.__new__(SearchArray)
        arr.avoid_copies, arr.tokenizer, arr._core, arr._rows = True, ws_tokenizer, _IndexCore(host), None
        frame = pd.DataFrame({"body": arr})
        qs = sets[0][:args.edismax_queries]
        for m in (2, 4):
            bt = new.index.batch(qs, k=K, min_match=[m] * len(qs))
            bt.run()
            _, want_rows = bt.fetch()
            bt.close()
            text = [" ".join(f"t{int(t)}" for t in q) for q in qs]
            edismax_search(frame, q=text[0], qf=["body"], mm=str(m), k=K)     # warm-up
            same = True
            t0 = time.perf_counter()
            for qi, q in enumerate(text):
                hits = edismax_search(frame, q=q, qf=["body"], mm=str(m), k=K)
                same = same and np.array_equal(np.asarray(hits.rows, dtype=np.uint64), want_rows[qi])
            dt = time.perf_counter() - t0
            ms_q = 1e3 * dt / len(text)
            emit({"leg": "c", "what": "edismax_search per query, one-column frame", "min_match": m, "k": K, "docs": D, "queries": len(text),
                  "ms_per_query": round(ms_q, 3), "rows_equal_leg_a": bool(same),
                  "ratio_c_to_a_per_query": round(ms_q / (a_ms[f"a/m={m}"] / B), 1)})
    out.close()
    for sd in sides:
        sd.close()


if __name__ == "__main__":
    main()
