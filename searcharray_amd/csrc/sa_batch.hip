// sa_batch.hip -- the host side of a top-k batch (Part 2 of the C ABI): the route rule of a BM25 batch, the upload image a
// query set is filled into, the shard run (plan, tables, run state, route launch, overflow check, merge), the exchange between
// ranks and the results.  The kernels and their launchers live in sa_bm25.hip, sa_stage.hip and sa_sparse.hip; a phrase batch
// fills and runs its shard in sa_phrase_batch.hip and shares the buffers, the run-state clear, the merge and the exchange.
#include "sa_index.hpp"
#include "sa_topk.hpp"
#include "sa_batch.hpp"
#include "sa_bm25_params.hpp"
#include "sa_facet.hpp"
#include "../../include/searcharray_hip.h"

#include <algorithm>
#include <new>
#include <stdlib.h>
#include <math.h>

// ---- the route rule of a BM25 batch
enum sa_route { SA_ROUTE_TILES, SA_ROUTE_GROUPED, SA_ROUTE_PRUNED, SA_ROUTE_STAGED };

struct sa_plan {
    bool group = false;          // the fill may group the rows for the grouped kernel
    bool seed_wanted = false;    // the fill derives starting bounds from the terms' rank tables
    bool stage_wanted = false;   // the fill plans the staged-tile route
    sa_route route = SA_ROUTE_TILES;   // per-query tile kernel, grouped overlay (+ the tile kernel), dynamic pruning, staged tiles
    bool imp = false;            // the kernels read the impact stream (else the TF postings)
    bool pruned = false;         // wave-level selection against a bound (else the block-level selection of every tile)
    bool hist = false;           // the histogram bound
    bool seed = false;           // the queries start with their starting bounds
    bool may_overflow = false;   // a candidate list can run over
};

// the tile sizes the grouped kernel and the impact-stream route are instantiated for
static bool sa_grouped_tiles(u32 tile_docs) { return tile_docs == 1024 || tile_docs == 2048 || tile_docs == 4096; }

// What a run of the batch's current query set does, from the batch, its index and its options alone (no side effects).
// sa_batch_fill asks it how to prepare the set, sa_batch_run_bm25 which route to launch.  `deferred`: an overflowing candidate
// list is only flagged on the device (sa_batch_run); `unpruned`: the redo of a flagged run.
static sa_plan sa_batch_plan(const sa_batch* bt, bool deferred, bool unpruned) {
    const sa_index* ix = bt->ix;
    const sa_options_t& o = bt->opts;
    sa_plan pl;
    // A batch with a document filter (sa_batch_set_filter) only ever takes a route that honours it: the staged-tile route, the grouped
    // overlay or the per-query tile kernels.  Dynamic pruning does not look at the filter, so the rule keeps a filtered batch off it
    // whatever the options say; and it starts without the rank-table bounds, which hold for the whole corpus only.
    const bool filtered = bt->filter != nullptr;
    // A batch with minimum-should-match values > 1 (sa_batch_set_min_match) is stricter still: only the per-query tile kernels count the
    // slots a doc matched, so its route is SA_ROUTE_TILES whatever the options say -- never staged, grouped or dynamically pruned -- and
    // it starts without the rank-table bounds, which count docs that the test may exclude.  The same holds for a batch with required or
    // prohibited slots (sa_batch_set_occur): the terms' rank tables know nothing of exclusions.
    const bool mm = bt->counting();
    // (the grouped kernel and the starting bounds need non-negative scores: the sign bit is a mark)
    pl.group = !mm && sa_opt(o.group, 1) != 0 && bt->weights_ok && sa_grouped_tiles(ix->tile_docs);   // (no row groups for a set that cannot take the overlay)
    pl.seed_wanted = bt->weights_ok && bt->impacts && bt->k <= 1024u && sa_opt(o.term_seed, 1) != 0 && sa_opt(o.sparse, -1) != 1;
    // the staged-tile route (sa_stage.hip) is asked for: option `stage` = 1, or unset while `sparse` is unset too (a caller that
    // sets `sparse` chooses between the two older routes)
    const long long stage_opt = sa_opt(o.stage, -1);
    pl.stage_wanted = stage_opt >= 0 ? stage_opt != 0 : !sa_opt_is_set(o.sparse);
    pl.imp = bt->impacts && sa_opt(o.impact, 1) != 0;
    pl.pruned = sa_opt(o.pruned_topk, 1) != 0 && !unpruned;     // pruned wave-level selection (any k <= 1024)
    const bool no_topk = sa_opt(o.no_topk, 0) != 0;
    // k > 32: histogram bound (BM25 tiles of <= 4 waves); topk_hist = 0 keeps the slot bound
    // dynamic pruning (sa_sparse.hip; sparse = 0: score every posting, the exhaustive reference
    // behaviour): needs the histogram bound for every k
    const bool hist_possible = pl.pruned && sa_tile_waves(ix->tile_docs) <= 8 && sa_opt(o.topk_hist, 1) != 0;
    // Round 5, measured instead of argued (scripts/route_rule.py, profiles/route_rule_r05*.jsonl: the share of the batch the grouped
    // kernel can take x k, 10 M and 1.25 M docs): with the impact stream and the starting bounds the exhaustive path is within 5 % of
    // pruning in EVERY cell and up to 2 x faster (k = 100, less than half of the batch groupable: 1.59 vs 2.92 ms -- round 4's rule
    // picked pruning there); pruning keeps the batches the impact route cannot take (no impact stream, the histogram bound off,
    // other tile sizes), where the per-query TF kernel is what it competes with.
    const bool impact_route = hist_possible && pl.imp && !no_topk && sa_grouped_tiles(ix->tile_docs);
    // Round 2: when most queries of the batch share their first terms, the grouped exhaustive kernel is as fast at
    // k = 10 and faster above (10 M docs, BASELINE batch: 369 K vs 341 K queries/s at k = 100, 236 K vs 114 K at
    // k = 1000) -- such batches score every posting from k = 32 on.
    // (only where the grouped kernel can actually run: impact stream, histogram bound, its tile sizes -- otherwise the
    //  batch would fall to the per-query exhaustive kernel, which pruning beats 2x)
    // Round 3: the grouped kernel (4 waves per SIMD, ~100 VALU instructions per (tile, query) pair) beats pruning on such
    // batches from k = 10 on (10 M docs, BASELINE batch, k = 10: 0.46 vs 0.63 ms per step) -- no lower limit on k any more.
    // ... and so do the loose groups on batches WITHOUT shared terms (256 x 4 pairwise-distinct terms of ranks 1 .. 1024,
    // all of them frequent: 0.62 ms exhaustive vs 1.68 ms pruned at k = 10): the exhaustive path is the default whenever
    // at least half of the batch's queries are in groups of either sort.
    // (the overlay's filtered instantiations exist for 1024- and 2048-doc tiles)
    const bool grouped = !mm && bt->n_groups && impact_route && sa_opt(o.group, 1) != 0 && !(filtered && ix->tile_docs > 2048u);
    // Unset, `sparse` follows the measurements: pruning pays while the shard holds many docs per requested
    // result (10 M docs: 2.2x at k = 10, 1.9x at k = 100, but the exhaustive kernel is 1.2x faster at k = 1000;
    // 1.25 M docs, k = 1000: exhaustive 1.8x faster) -- on from 32768 docs per result (8192 since round 6, below).  sparse = 1 / 0 force it.
    // Round 6, the batches that remain (no impact stream), measured by shard size (profiles/route_rule_r06_no_impact_stream*.jsonl: 1.25 / 2.5 /
    // 5 / 10 M docs x k = 10 / 100 / 1000 x two query sets): pruning beats the TF kernels 1.4 - 5.7 x from 10 000 docs per requested result
    // on (1.0 - 1.9 x at 10 000 - 12 500), loses up to 1.4 x at 5 000 and below -- on from 8192 docs per result (rounds 3-5: 32768).
    const long long sparse_opt = sa_opt(o.sparse, -1);
    const bool sparse_wanted = sparse_opt >= 0 ? sparse_opt != 0 : (ix->n_docs >= (u64)bt->k * 8192ull && !impact_route);
    // Round 6: the staged-tile route (sa_stage.hip) takes every query set it has a plan for -- distinct terms staged in LDS once
    // per tile, the queries answered from there; it needs the histogram bound and the impact stream like the grouped kernel
    const bool stage = !mm && bt->stage_ok && pl.stage_wanted && hist_possible && pl.imp && !no_topk && ix->avg_doc_len != 0.f;
    const bool sparse = !stage && !filtered && !mm && sparse_wanted && hist_possible && ix->tile_docs <= 8192 && ix->avg_doc_len != 0.f && ix->n_tiles > 0;
    // (a run that checks overflow on the host keeps the slot bound up to k = 32)
    pl.hist = hist_possible && (sparse || stage || deferred || bt->k > 32);
    pl.route = stage ? SA_ROUTE_STAGED : sparse ? SA_ROUTE_PRUNED : grouped && pl.hist ? SA_ROUTE_GROUPED : SA_ROUTE_TILES;
    // the bounds the queries start with (exhaustive kernels only: the pruning path derives its own from the lead terms)
    pl.seed = pl.hist && !sparse && bt->seed_on && pl.imp && !filtered && !mm;
    // (with the histogram bound a wave appends all its survivors, so the worst case is not bounded by k)
    pl.may_overflow = pl.pruned && (bt->cap_limited || pl.hist) && ix->n_tiles > 0;
    return pl;
}

// the slice table of the batch's current query set (the staged-tile route leaves it out of the step: built when another route runs)
static int sa_batch_ensure_bounds(sa_batch* bt, hipStream_t st) {
    if (bt->bounds_valid) return SA_OK;
    SA_TRY(sa_launch_make_bounds(bt->ix, bt->d_terms, bt->B * bt->T, bt->d_bounds, bt->d_qbase, st, bt->d_qbase_imp,
                                 bt->seed_on ? bt->impacts->d_topf : nullptr, bt->d_idf, bt->T, bt->k, bt->d_seed,
                                 (float)sa_opt(bt->opts.seed_scale_pct, 100) / 100.f));
    bt->bounds_valid = true;
    return SA_OK;
}

void sa_batch_free(sa_batch* bt) {
    if (!bt) return;
    if (bt->ix) {
        // every stream a run of this batch may have used: the index stream, the side stream (ungrouped rows), the
        // exchange stream (all-gather, cross-rank merge, result copies) and the lanes of dense-route phrases
        hipSetDevice(bt->ix->device);
        hipStreamSynchronize(bt->ix->stream);
        if (bt->st) hipStreamSynchronize(bt->st);
        if (bt->ix->sstream) hipStreamSynchronize(bt->ix->sstream);
        if (bt->ix->xstream) hipStreamSynchronize(bt->ix->xstream);
        for (int j = 0; j < 3; j++)
            if (bt->ix->lane_stream[j]) hipStreamSynchronize(bt->ix->lane_stream[j]);
    }
    // (d_terms, d_idf, d_perm, d_grp, d_ub, d_ub_order, d_lead, d_p1_off, d_qdf, d_qrow8, d_bloom_off, d_bloom_shift,
    //  d_plan live inside the upload block)
    if (bt->own_stream && bt->st) { hipStreamSynchronize(bt->st); hipStreamDestroy(bt->st); }
    if (bt->d_up) hipFree(bt->d_up);
    for (int i = 0; i < 2; i++) {
        if (bt->h_up[i]) hipHostFree(bt->h_up[i]);
        if (bt->ev_up[i]) hipEventDestroy(bt->ev_up[i]);
    }
    if (bt->h_res) hipHostFree(bt->h_res);
    if (bt->ev_res) hipEventDestroy(bt->ev_res);
    if (bt->ev_final) hipEventDestroy(bt->ev_final);
    if (bt->d_cand) hipFree(bt->d_cand);
    if (bt->d_bounds) hipFree(bt->d_bounds);
    if (bt->d_sattab) hipFree(bt->d_sattab);
    if (bt->d_qbase) hipFree(bt->d_qbase);
    if (bt->d_qbase_imp) hipFree(bt->d_qbase_imp);
    bt->impacts.reset();
    if (bt->d_slots) hipFree(bt->d_slots);
    if (bt->d_local) hipFree(bt->d_local);
    if (bt->d_gather) hipFree(bt->d_gather);
    if (bt->d_xlocal) hipFree(bt->d_xlocal);
    for (int i = 0; i < 2; i++) {
        if (bt->ev_side[i]) hipEventDestroy(bt->ev_side[i]);
        if (bt->ev_scored[i]) hipEventDestroy(bt->ev_scored[i]);
        if (bt->ev_exchanged[i]) hipEventDestroy(bt->ev_exchanged[i]);
    }
    if (bt->d_final) hipFree(bt->d_final);
    if (bt->d_xcand) hipFree(bt->d_xcand);
    if (bt->d_wbounds) hipFree(bt->d_wbounds);
    if (bt->d_wbase) hipFree(bt->d_wbase);
    if (bt->d_wlen) hipFree(bt->d_wlen);
    if (bt->d_stats) hipFree(bt->d_stats);
    if (bt->d_facet) hipFree(bt->d_facet);
    if (bt->d_wl) hipFree(bt->d_wl);
    if (bt->d_wl_cnt) hipFree(bt->d_wl_cnt);
    if (bt->d_iota) hipFree(bt->d_iota);
    if (bt->d_route) hipFree(bt->d_route);
    if (bt->d_emask) hipFree(bt->d_emask);
    if (bt->d_p2_off) hipFree(bt->d_p2_off);
    if (bt->d_tile_q) hipFree(bt->d_tile_q);
    if (bt->d_surv) hipFree(bt->d_surv);
    if (bt->d_bloom) hipFree(bt->d_bloom);
    for (hipEvent_t e : bt->ev0) hipEventDestroy(e);
    for (hipEvent_t e : bt->ev1) hipEventDestroy(e);
    delete bt;
}

// The upload block of a batch: `bytes` on the device + two page-locked host images (see sa_batch.hpp).
int sa_batch_alloc_upload(sa_batch* bt, size_t bytes) {
    bt->up_bytes = (bytes + 15) & ~(size_t)15;
    SA_HIP(hipMalloc(&bt->d_up, bt->up_bytes));
    for (int i = 0; i < 2; i++) {
        SA_HIP(hipHostMalloc(&bt->h_up[i], bt->up_bytes, 0));
        memset(bt->h_up[i], 0, bt->up_bytes);
        SA_HIP(hipEventCreateWithFlags(&bt->ev_up[i], hipEventDisableTiming));
    }
    return SA_OK;
}

// The host image the next reset fills (waits, if it must, until the copy that last used it is done -- two resets
// ago, so in a steady stream this never blocks).
int sa_batch_upload_begin(sa_batch* bt, char** image) {
    const u32 i = bt->up_n & 1u;
    if (bt->up_used[i]) SA_HIP(hipEventSynchronize(bt->ev_up[i]));
    *image = bt->h_up[i];
    return SA_OK;
}

// one async copy of the whole image, on the index stream: ordered behind the runs that still read the old tables
int sa_batch_upload_commit(sa_batch* bt) {
    const u32 i = bt->up_n & 1u;
    SA_HIP(hipMemcpyAsync(bt->d_up, bt->h_up[i], bt->up_bytes, hipMemcpyHostToDevice, bt->st));
    SA_HIP(hipEventRecord(bt->ev_up[i], bt->st));
    bt->up_used[i] = true;
    bt->up_n++;
    return SA_OK;
}

// Candidate lists, pruning slots, result buffers and the timing-event ring of a batch whose tile
// kernel runs n_tiles tiles of `waves` waves per query; a candidate list holds at least `min_cap` keys.
int sa_batch_alloc_topk(sa_batch* bt, u32 n_tiles, u32 waves, u64 min_cap) {
    const u32 B = bt->B;
    // candidate storage per query: worst case every wave appends k keys; capped at 1 Mi keys per
    // query (8 MiB) -- with the cap an overflow is theoretically possible and is detected at run
    // time (sa_batch_run_bm25 re-runs a BM25 batch with the unpruned block-level selection).
    const u64 worst = (u64)(n_tiles ? n_tiles : 1) * bt->k * waves;
    const u64 mode0 = (u64)(n_tiles ? n_tiles : 1) * bt->k;
    u64 cap = worst < (1ull << 20) ? worst : (1ull << 20);
    if (cap < mode0) cap = mode0;                      // the unpruned layout [n_tiles][k] must fit too
    if (cap < min_cap) cap = min_cap;
    if (sa_opt_is_set(bt->opts.cand_cap)) {            // tests: force the overflow handling
        const u64 forced = (u64)bt->opts.cand_cap;
        cap = forced > mode0 ? forced : mode0;
    }
    bt->cand_cap = (u32)cap;
    bt->cap_limited = cap < worst;                     // (sa_tile_topk_pruned appends at most k keys per wave)
    const size_t ncand = (size_t)B * cap;
    SA_HIP(hipMalloc(&bt->d_cand, ncand * sizeof(u64)));
    // slots + cursors (+ cached bounds + score histograms for k > 32): one memset per run
    SA_HIP(hipMalloc(&bt->d_slots, ((size_t)B * (34 + SA_HBINS) + 1) * sizeof(u32)));
    bt->d_cand_cnt = bt->d_slots + (size_t)B * 32;
    bt->d_gthr = bt->d_slots + (size_t)B * 33;
    bt->d_hist = bt->d_slots + (size_t)B * 34;
    SA_HIP(hipMalloc(&bt->d_local, (size_t)B * bt->k * sizeof(u64)));
    // the final keys, and behind them two flag cells that travel to the host with them in ONE copy: [B*k] "a candidate
    // list of this shard ran over" (set by the merge kernel), [B*k + 1] the same over all ranks (set by the exchange)
    SA_HIP(hipMalloc(&bt->d_final, ((size_t)B * bt->k + 2) * sizeof(u64)));
    SA_HIP(hipMemset(bt->d_final, 0, ((size_t)B * bt->k + 2) * sizeof(u64)));
    bt->d_overflow = (u32*)(bt->d_final + (size_t)B * bt->k);
    bt->d_xflag = (u32*)(bt->d_final + (size_t)B * bt->k + 1);
    SA_HIP(hipMemset(bt->d_local, 0, (size_t)B * bt->k * sizeof(u64)));
    SA_HIP(hipHostMalloc(&bt->h_res, ((size_t)B * bt->k + 2) * sizeof(u64), 0));
    SA_HIP(hipEventCreateWithFlags(&bt->ev_res, hipEventDisableTiming));
    SA_HIP(hipEventCreateWithFlags(&bt->ev_final, hipEventDisableTiming));
    for (int i = 0; i < SA_EVENT_RING; i++) {
        hipEvent_t a = nullptr, c = nullptr;
        SA_HIP(hipEventCreate(&a));
        bt->ev0.push_back(a);
        SA_HIP(hipEventCreate(&c));
        bt->ev1.push_back(c);
    }
    return SA_OK;
}

static u64 sa_pow2_cells(u64 df) {                     // Bloom cells of a lead term: the power of two in [8, 16) x df, at least 1024
    u32 bits = 10;
    while ((1ull << bits) < 8 * df && bits < 30) bits++;
    return 1ull << bits;
}

// ---- a BM25 batch in two steps: sa_batch_alloc_bm25 sizes every device buffer ONCE from (B, T, k, the shard's
//      tiles), sa_batch_fill computes everything that depends on the queries into the upload image and enqueues the
//      copy and the slice-table kernel.  sa_batch_create = alloc + fill + one synchronisation; sa_batch_reset = fill.
static int sa_batch_alloc_bm25(sa_batch* bt) {
    sa_index* ix = bt->ix;
    const size_t B = bt->B, T = bt->T;
    // A BM25 batch has a stream of its own: batches of one index share nothing but the (read-only) index, so two
    // batches used alternately by a query stream overlap -- the tail of one batch's scoring kernels (the last, partly
    // filled round of workgroups) and its merge run beside the head of the next.
    SA_HIP(hipStreamCreateWithFlags(&bt->st, hipStreamNonBlocking));
    bt->own_stream = true;
    // upload block (8-byte fields first)
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 7) & ~(size_t)7; return o; };
    const size_t o_p1 = take((B + 1) * 8), o_boff = take(B * 8), o_terms = take(B * T * 4), o_idf = take(B * T * 4),
                 o_perm = take(B * 4), o_grp = take(3 * B * 4), o_ub = take(B * (T + 1) * 4), o_ord = take(B * T * 4),
                 o_lead = take(B * 4), o_qdf = take(B * T * 4), o_row8 = take(B * T * 4), o_bsh = take(B * 4),
                 o_seed = take(B * 4);
    bt->st_bytes = sa_stage_upload_bytes((u32)B, (u32)T);
    off = (off + 15) & ~(size_t)15;
    const size_t o_st = take(bt->st_bytes);
    const size_t o_mm = take(B * 4), o_occ = take(B * 8);
    SA_TRY(sa_batch_alloc_upload(bt, off));
    char* u = bt->d_up;
    bt->d_p1_off = (u64*)(u + o_p1); bt->d_bloom_off = (u64*)(u + o_boff);
    bt->d_terms = (u32*)(u + o_terms); bt->d_idf = (float*)(u + o_idf); bt->d_perm = (u32*)(u + o_perm);
    bt->d_grp = (u32*)(u + o_grp); bt->d_ub = (float*)(u + o_ub); bt->d_ub_order = (u32*)(u + o_ord);
    bt->d_lead = (u32*)(u + o_lead); bt->d_qdf = (u32*)(u + o_qdf); bt->d_qrow8 = (u32*)(u + o_row8);
    bt->d_bloom_shift = (u32*)(u + o_bsh);
    bt->d_seed = (u32*)(u + o_seed);
    bt->d_st = u + o_st;
    bt->d_min_match = (u32*)(u + o_mm);              // (behind d_terms: Bm25Params::min_match_off)
    bt->d_occur = (u32*)(u + o_occ);                 // (likewise: Bm25Params::occur_off)
    {
        std::vector<u32> iota(B);
        for (u32 i = 0; i < B; i++) iota[i] = i;
        SA_HIP(hipMalloc(&bt->d_iota, B * sizeof(u32)));
        SA_HIP(hipMemcpy(bt->d_iota, iota.data(), B * sizeof(u32), hipMemcpyHostToDevice));
    }
    // work list of the grouped kernel: at most one entry per (tile, row)
    bt->wl_cap = (u32)std::max<size_t>(1, (size_t)ix->n_tiles * B);
    SA_HIP(hipMalloc(&bt->d_wl, (size_t)bt->wl_cap * sizeof(u64)));
    SA_HIP(hipMalloc(&bt->d_wl_cnt, sizeof(u32)));
    SA_HIP(hipMemset(bt->d_wl_cnt, 0, sizeof(u32)));
    // (the sparse candidate path appends every doc of a lead term that is scored before the bound exists)
    SA_TRY(sa_batch_alloc_topk(bt, ix->n_tiles, sa_tile_waves(ix->tile_docs), 1ull << 17));
    SA_HIP(hipMalloc(&bt->d_bounds, (B * T * (ix->n_tiles + 1) + 1) * sizeof(u32)));
    SA_HIP(hipMalloc(&bt->d_qbase, B * T * sizeof(u64)));
    SA_HIP(hipMalloc(&bt->d_sattab, SA_SAT_NTF * SA_SAT_WMAX * sizeof(float)));
    // dynamic pruning (sa_sparse.hip): device-only tables
    SA_HIP(hipMalloc(&bt->d_route, B * sizeof(u32)));
    SA_HIP(hipMalloc(&bt->d_emask, B * sizeof(u32)));
    SA_HIP(hipMalloc(&bt->d_p2_off, (B + 1) * sizeof(u64)));
    SA_HIP(hipMalloc(&bt->d_tile_q, (B + 2) * sizeof(u32)));
    SA_HIP(hipMemset(bt->d_route, 0xFF, B * sizeof(u32)));
    {
        // survivors of the phase-2 bound check: a few percent of the candidates; capped, the rest is scored in place
        u64 cap = (u64)B * 65536;
        if (cap > (16u << 20)) cap = 16u << 20;
        bt->surv_cap = (u32)cap;
        SA_HIP(hipMalloc(&bt->d_surv, (size_t)cap * 2 * sizeof(u64)));
    }
    SA_TRY(sa_launch_make_sattab(ix, bt->d_sattab, &bt->tab_w, bt->k1, bt->b, bt->st));
    // the impact stream of this (k1, b): shared through the index, built on first use (on the index stream: done
    // before this batch's stream goes on)
    bt->impacts = sa_impacts_get(ix, bt->k1, bt->b, bt->opts);
    SA_HIP(hipStreamSynchronize(ix->stream));
    if (bt->impacts) SA_HIP(hipMalloc(&bt->d_qbase_imp, B * T * 2 * sizeof(u64)));
    return SA_OK;
}

// lead terms of dynamic pruning: up to 1/64 of the shard's docs (phase 1 scores every one of them), and never more
// postings than fit the candidate list while the bound is still unknown
static u64 sa_batch_lead_limit(const sa_batch* bt) {
    const sa_index* ix = bt->ix;
    u64 limit1 = ix->n_docs / 64 > 4096 ? ix->n_docs / 64 : 4096;
    if (limit1 > (u64)bt->cand_cap * 3 / 4) limit1 = (u64)bt->cand_cap * 3 / 4;
    return limit1;
}

// The Bloom filters of the lead terms are sized per query set (bt->bloom_bytes, sa_batch_fill).  The buffer holds what the
// query sets seen so far needed, with half as much again: a run whose set needs more waits for the batch's stream (older runs
// of this batch read the old buffer), frees it and allocates the larger one -- after the first few sets of a stream never
// again.  (Round 3 allocated the worst case of the shard -- B lead terms of lead-limit postings each: 512 MiB per 256-query
// batch at 10 M docs where a BASELINE set needs ~20 MiB.)
int sa_batch_ensure_bloom(sa_batch* bt) {
    const size_t need = bt->bloom_bytes;
    if (bt->d_bloom && bt->bloom_cap >= need) return SA_OK;
    if (bt->d_bloom) {
        SA_HIP(hipStreamSynchronize(bt->st));
        SA_HIP(hipFree(bt->d_bloom));
        bt->d_bloom = nullptr; bt->bloom_cap = 0;
    }
    size_t cap = need + need / 2;
    const size_t floor_bytes = (size_t)std::max<long long>(1024, sa_opt(bt->opts.bloom_floor, 1 << 20));      // (tests: small, so that the buffer has to grow)
    if (cap < floor_bytes) cap = floor_bytes;
    SA_HIP(hipMalloc(&bt->d_bloom, cap));
    bt->bloom_cap = cap;
    return SA_OK;
}

// Dynamic pruning tables of the current query set (sa_sparse.hip), derived into the upload image `img` from the rows already
// placed there (terms / idf in device-row order).  ~9 us for 256 x 4 terms: sa_batch_fill only calls it when the route rule
// (sa_batch_plan) sends the run down the pruning path; a run that takes the path after all -- an option changed between reset
// and run -- derives them then and uploads the image again (sa_batch_ensure_tables).
static void sa_batch_fill_prune_tables(sa_batch* bt, char* img) {
    sa_index* ix = bt->ix;
    const u32 B = bt->B, T = bt->T;
    const float k1 = bt->k1, b = bt->b;
    auto at = [&](const void* dptr) { return img + ((const char*)dptr - bt->d_up); };
    u64* h_p1 = (u64*)at(bt->d_p1_off);
    u64* h_boff = (u64*)at(bt->d_bloom_off);
    u32* h_terms = (u32*)at(bt->d_terms);
    float* h_idf = (float*)at(bt->d_idf);
    float* h_ub = (float*)at(bt->d_ub);
    u32* h_ord = (u32*)at(bt->d_ub_order);
    u32* h_lead = (u32*)at(bt->d_lead);
    u32* h_qdf = (u32*)at(bt->d_qdf);
    u32* h_row8 = (u32*)at(bt->d_qrow8);
    u32* h_bshift = (u32*)at(bt->d_bloom_shift);
        // Dynamic pruning tables (sa_sparse.hip).  Per query: the terms in ascending idf order with the
        // prefix sums of their idf -- what the j cheapest terms can add to a score at most, since
        // tf/(tf+norm) <= 1 (needs k1 >= 0 and 0 <= b <= 1; a negative or non-finite idf switches the
        // pruning off) -- and the LEAD term: the highest-idf term with postings in this shard.
        const bool formula_ok = k1 >= 0.f && b >= 0.f && b <= 1.f;
        const u64 limit1 = sa_batch_lead_limit(bt);
        const u64 sp_div = (u64)std::max<long long>(1, sa_opt(bt->opts.sparse_div, 8));
        bt->sparse_limit2 = ix->n_docs / sp_div > 4096 ? ix->n_docs / sp_div : 4096;
        std::pair<float, u32> v[SA_MAX_QTERMS];
        h_p1[0] = 0;
        for (u32 r = 0; r < B; r++) {
            bool ok = formula_ok;
            for (u32 t = 0; t < T; t++) {
                const bool known = h_terms[(size_t)r * T + t] < ix->n_terms;
                const float w = known ? h_idf[(size_t)r * T + t] : 0.f;
                if (!(w >= 0.f) || w > 3.0e38f) ok = false;
                v[t] = {w, t};
            }
            std::stable_sort(v, v + T, [](const std::pair<float, u32>& a, const std::pair<float, u32>& c) { return a.first < c.first; });
            double acc = 0.0;
            h_ub[(size_t)r * (T + 1)] = 0.f;
            for (u32 j = 0; j < T; j++) {
                h_ord[(size_t)r * T + j] = v[j].second;
                acc += (double)v[j].first;
                // rounded up: the fp32 sum the kernels form can exceed the exact sum by a few ulps
                float ubf = (float)(acc * (1.0 + 1e-5));
                ubf = nextafterf(ubf, INFINITY);
                h_ub[(size_t)r * (T + 1) + j + 1] = ok ? ubf : INFINITY;
            }
            // lead: highest idf among the terms with postings here; too frequent -> scan the tiles
            h_lead[r] = 0xFFFFFFFFu;
            h_p1[r + 1] = 0;
            if (ok) {
                for (int j = (int)T - 1; j >= 0; j--) {
                    const u32 t = v[(size_t)j].second;
                    const u32 term = h_terms[(size_t)r * T + t];
                    if (term >= ix->n_terms) continue;
                    const u64 df = ix->h_tf_off[term + 1] - ix->h_tf_off[term];
                    if (df == 0) continue;
                    if (df <= limit1) { h_lead[r] = t; h_p1[r + 1] = df; }          // postings; turned into items below
                    break;
                }
            }
        }
        {
            // Lead-phase work items: 1024 postings each when there is plenty of work (measured best at
            // 10 M docs: 0.66 vs 0.79 ms per step with 256), 256 when the shard is small and the phase
            // would otherwise not fill the GPU (1.25 M docs: 0.157 vs 0.169 ms).
            u64 lead_postings = 0;
            for (u32 r = 0; r < B; r++) lead_postings += h_p1[r + 1];
            bt->sparse_chunk1 = lead_postings >= (1ull << 19) ? SA_SP_CHUNK : SA_SP_CHUNK_LEAD;
            if (sa_opt(bt->opts.sp_chunk1, 0) >= 64) bt->sparse_chunk1 = (u32)bt->opts.sp_chunk1;
            for (u32 r = 0; r < B; r++) h_p1[r + 1] = (h_p1[r + 1] + bt->sparse_chunk1 - 1) / bt->sparse_chunk1;
        }
        for (u32 r = 0; r < B; r++) h_p1[r + 1] += h_p1[r];
        bt->sparse_p1_total = h_p1[B];
        bt->sparse_ok = true;
        bt->sparse_p2_max = 0;
        for (size_t i = 0; i < (size_t)B * T; i++) {
            const u32 term = h_terms[i];
            h_qdf[i] = 0; h_row8[i] = SA_DD_NONE;
            if (term >= ix->n_terms) continue;
            h_qdf[i] = (u32)(ix->h_tf_off[term + 1] - ix->h_tf_off[term]);
            bt->sparse_p2_max += ((u64)h_qdf[i] + SA_SP_CHUNK - 1) / SA_SP_CHUNK;
            if (!ix->h_tf8_slot.empty()) h_row8[i] = ix->h_tf8_slot[term];
        }
        // Bloom filter of every lead term: the power of two in [8, 16) x df cells, at least 1024
        size_t bytes = 0;
        for (u32 r = 0; r < B; r++) {
            const u64 df = h_lead[r] == 0xFFFFFFFFu ? 0 : h_qdf[(size_t)r * T + h_lead[r]];
            const u64 cells = sa_pow2_cells(df);
            h_boff[r] = bytes;
            h_bshift[r] = 32u - (u32)__builtin_ctzll(cells);
            bytes += (size_t)cells;
        }
        bt->bloom_bytes = bytes;
}

// ---- a query set into the upload image (sa_batch_fill): row order, groups, starting bounds, the staged-tile plan, the pruning
//      tables where the run will prune, the copy

// Order queries by their most frequent term so XCD groups share posting tiles in L2 (bt->perm: device row -> caller query;
// and the set's byte counts, sa_batch_profile).
static void sa_batch_order_rows(sa_batch* bt, const u32* terms) {
    sa_index* ix = bt->ix;
    const u32 B = bt->B, T = bt->T;
    bt->perm.resize(B);
    for (u32 i = 0; i < B; i++) bt->perm[i] = i;
    std::vector<u64> heavy(B, 0);
    std::vector<u32> heavy_term(B, SA_NO_TERM);
    bt->alg_bytes = 0; bt->postings_bytes = 0;
    for (u32 i = 0; i < B; i++) {
        for (u32 t = 0; t < T; t++) {
            const u32 term = terms[(size_t)i * T + t];
            if (term >= ix->n_terms) continue;
            const u64 df = ix->h_tf_off[term + 1] - ix->h_tf_off[term];
            bt->postings_bytes += 8 * df;
            if (df > heavy[i]) { heavy[i] = df; heavy_term[i] = term; }
        }
        bt->alg_bytes += 4 * ix->n_docs;
    }
    bt->alg_bytes += bt->postings_bytes;
    std::stable_sort(bt->perm.begin(), bt->perm.end(), [&](u32 a, u32 c) {
        if (heavy[a] != heavy[c]) return heavy[a] > heavy[c];
        return heavy_term[a] < heavy_term[c];
    });
}

// Loose groups: queries left over whose terms are all sparse per tile (what a (tile, query) pair of the
// per-query kernel costs is clearing and scanning the tile's accumulators, 2048 slots for ~130 postings;
// as an overlay on accumulators that are cleared once per 16 queries and touched only where the postings
// are, it costs the postings).  Eligible: an expected sum of postings per tile that fits the overlay's
// half table with room to spare; the others keep the per-query kernel (their tiles are dense).  Moves the
// queries it groups from `rest` to `order`; false when it forms none.
static bool sa_batch_group_loose(sa_batch* bt, const u32* terms, u32 item_q, std::vector<u32>& rest, std::vector<u32>& order,
                                 std::vector<u32>& h_grp) {
    const sa_index* ix = bt->ix;
    const u32 T = bt->T;
    std::vector<u32> sparse_rows, dense_rows;
    for (u32 q : rest) {
        u64 dfsum = 0;
        for (u32 t = 0; t < T; t++) {
            const u32 term = terms[(size_t)q * T + t];
            if (term < ix->n_terms) dfsum += ix->h_tf_off[term + 1] - ix->h_tf_off[term];
        }
        if (dfsum > 0 && dfsum / ix->n_tiles <= (u64)std::max<long long>(1, sa_opt(bt->opts.loose_postings, SA_GRP_LOOSE_POSTINGS))) sparse_rows.push_back(q);
        else dense_rows.push_back(q);
    }
    if (sparse_rows.size() < 2) return false;
    const u32 item_l = sa_opt_is_set(bt->opts.group_item) ? std::max<u32>(SA_GRP_MAXQ, item_q / SA_GRP_MAXQ * SA_GRP_MAXQ) : (u32)SA_GRP_MAXQ;
    const u32 pieces = ((u32)sparse_rows.size() + item_l - 1) / item_l;
    u32 done = 0;
    for (u32 pc = 0; pc < pieces; pc++) {
        const u32 sz = ((u32)sparse_rows.size() - done + (pieces - pc) - 1) / (pieces - pc);
        h_grp.push_back((u32)order.size()); h_grp.push_back(sz | 0x80000000u); h_grp.push_back(0xFFFFFFFFu);
        for (u32 i = 0; i < sz; i++) order.push_back(sparse_rows[done + i]);
        done += sz;
    }
    rest = dense_rows;
    return true;
}

// Groups of ONE (round 6, option group_one; round 5 review item 4): a query left over -- too dense for a loose group, its first
// term shared with nobody -- is an item of its own: one WAVE per (tile, query) whose base comes from the first term's dense factor
// row with 16-byte loads where it has one (no scatter of ~1900 postings per tile), from its postings otherwise, the other terms
// overlaid.  Without it such queries run the per-query kernel (a workgroup per pair) on the side stream.  Measured
// (profiles/group_of_one_dense_row_ab_r06.jsonl; 256 pairwise-distinct queries, 13 of them left over, 10 with a dense row):
// 10 M docs k = 10 / 1000: none 0.465 / 0.859 ms, rows only (group_one = 1) 0.431 / 0.725, all (2, the default) 0.408 / 0.648;
// 1.25 M docs k = 10 / 100: 0.138 / 0.180 -> 0.106 / 0.132; never slower on the BASELINE / hot sets.
static void sa_batch_group_ones(sa_batch* bt, const u32* terms, std::vector<u32>& rest, std::vector<u32>& order, std::vector<u32>& h_grp) {
    const sa_index* ix = bt->ix;
    const long long g1 = sa_opt(bt->opts.group_one, 2);
    if (g1 == 0 || !bt->impacts || sa_opt(bt->opts.group_dense, 1) == 0) return;
    std::vector<u32> still;
    for (u32 q : rest) {
        const u32 t0 = terms[(size_t)q * bt->T];
        const u32 slot = (bt->impacts->d_dense && t0 < ix->n_terms && t0 < bt->impacts->dense_slot.size()) ? bt->impacts->dense_slot[t0] : 0xFFFFFFFFu;
        if (slot != 0xFFFFFFFFu || (g1 >= 2 && t0 < ix->n_terms)) { h_grp.push_back((u32)order.size()); h_grp.push_back(1u); h_grp.push_back(slot); order.push_back(q); }
        else still.push_back(q);
    }
    rest = still;
}

// Groups of queries that share their FIRST term (same term, same idf bits): sa_k_bm25_group_tiles scores the
// shared term once per (tile, group).  Grouped queries take the first device rows, group by group (big
// groups are cut into balanced pieces of at most `maxq` queries), the others keep their order behind them.
// `on`: the query set may be grouped (sa_batch_plan).  Reorders bt->perm; the group table [first row, rows, dense factor row]
// goes to h_grp.
static void sa_batch_group_rows(sa_batch* bt, const u32* terms, const float* idf, bool on, std::vector<u32>& h_grp) {
    sa_index* ix = bt->ix;
    const u32 B = bt->B, T = bt->T;
    bt->n_groups = 0; bt->n_grouped_rows = 0; bt->n_shared_rows = 0;
    // lanes per query while the half tables are built: a power of two >= the terms overlaid -- T - 1 for groups
    // with a shared first term, T for loose groups (decided below; loose groups are only formed if the wider
    // table still takes SA_GRP_MAXQ queries)
    u32 tt = 1, tsh = 0;
    while (tt + 1u < T) { tt <<= 1; tsh++; }               // power of two >= max(T - 1, 1)
    u32 tt_loose = 1, tsh_loose = 0;
    while (tt_loose < T) { tt_loose <<= 1; tsh_loose++; }
    const bool loose_on = sa_opt(bt->opts.group_loose, 1) != 0 && 128u / tt_loose >= SA_GRP_MAXQ;
    u32 maxq = std::min<u32>(SA_GRP_MAXQ, 128u / tt);
    // (a shard whose (tile, group) items do not fill the device for many rounds is better cut into more, shorter items:
    //  SA_GROUP_MAXQ; measured on a 1.25 M-doc shard below)
    maxq = std::min<u32>(maxq, (u32)std::max<long long>(1, sa_opt(bt->opts.group_maxq, SA_GRP_MAXQ)));
    // queries per ITEM: an item takes its queries in passes of maxq over one base, so a group of 25 is ONE item (two passes), not
    // two items that each pay the item's fixed cost (block -> tile, group entry, slice of the shared term, dense row, base:
    // ~6 K of an item's ~34 K cycles)
    //  Two passes per item are worth it where the launch has many rounds of items to run (same box, BASELINE batch, items of 16 vs
    //  32 queries: 10 M docs 0.402 -> 0.381 ms, 7.5 M 0.311 -> 0.302, 5 M 0.2185 -> 0.218, 2.5 M 0.124 -> 0.134, 1.25 M 0.085 -> 0.094:
    //  fewer, longer items lengthen the launch's tail) -- from 16 rounds of the device's 4096 resident waves on; loose groups have
    //  no base to share and keep 16 (measured: 0.464 -> 0.483 ms with 32).  2048 queries per batch (groups of ~200, 155 rounds): items of
    //  16 / 32 / 48 / 64 queries 2.339 / 2.213 / 2.172 / 2.168 ms -- four passes from 64 rounds on.
    u32 item_q = maxq;                                      // (set below, once the groups are known)
    bt->grp_cq = maxq;
    const u32 gmin = (u32)std::max<long long>(1, sa_opt(bt->opts.group_min, 2));
    if (on) {
        std::vector<std::vector<u32>> members;              // in order of first appearance
        std::vector<std::pair<u32, u32>> keys;
        std::vector<u32> rest;
        for (u32 r = 0; r < B; r++) {
            const u32 q = bt->perm[r];
            const u32 t0 = terms[(size_t)q * T];
            u32 ib; memcpy(&ib, &idf[(size_t)q * T], 4);
            if (t0 >= ix->n_terms) { rest.push_back(q); continue; }
            size_t gi = 0;
            for (; gi < keys.size(); gi++) if (keys[gi].first == t0 && keys[gi].second == ib) break;
            if (gi == keys.size()) { keys.push_back({t0, ib}); members.emplace_back(); }
            members[gi].push_back(q);
        }
        {
            u64 items16 = 0;
            for (auto& m : members) if (m.size() >= gmin) items16 += (m.size() + maxq - 1) / maxq;
            const u64 rounds = items16 * (u64)ix->n_tiles / 4096u;          // of one-pass items over the device's resident waves
            const long long dflt = rounds >= 4u * SA_GRP_ITEM_ROUNDS ? 64 : rounds >= (u64)SA_GRP_ITEM_ROUNDS ? 32 : 16;
            item_q = std::max<u32>(maxq, std::min<u32>(64u, (u32)std::max<long long>(1, sa_opt(bt->opts.group_item, dflt))) / maxq * maxq);
        }
        std::vector<u32> order;
        for (auto& m : members) {
            if (m.size() < gmin) { rest.insert(rest.end(), m.begin(), m.end()); continue; }
            const u32 pieces = ((u32)m.size() + item_q - 1) / item_q;
            u32 done = 0;
            for (u32 pc = 0; pc < pieces; pc++) {
                const u32 sz = ((u32)m.size() - done + (pieces - pc) - 1) / (pieces - pc);
                h_grp.push_back((u32)order.size()); h_grp.push_back(sz);
                {
                    const u32 t0 = terms[(size_t)m[done] * T];
                    const bool have = bt->impacts && bt->impacts->d_dense && t0 < bt->impacts->dense_slot.size();
                    h_grp.push_back(have ? bt->impacts->dense_slot[t0] : 0xFFFFFFFFu);
                }
                for (u32 i = 0; i < sz; i++) order.push_back(m[done + i]);
                done += sz;
            }
        }
        bt->n_shared_rows = (u32)order.size();                   // rows in groups with a shared first term
        if (loose_on && ix->n_tiles > 0 && sa_batch_group_loose(bt, terms, item_q, rest, order, h_grp)) { tt = tt_loose; tsh = tsh_loose; }
        sa_batch_group_ones(bt, terms, rest, order, h_grp);
        bt->n_grouped_rows = (u32)order.size();
        bt->n_groups = (u32)(h_grp.size() / 3);
        order.insert(order.end(), rest.begin(), rest.end());
        bt->perm = order;
    }
    bt->grp_tt = tt; bt->grp_tt_shift = tsh;
}

static int sa_batch_fill(sa_batch* bt, const uint32_t* terms, const float* idf) {
    sa_index* ix = bt->ix;
    const u32 B = bt->B, T = bt->T;
    char* img = nullptr;
    const u64 t_begin = sa_now_ns();
    SA_TRY(sa_batch_upload_begin(bt, &img));
    auto at = [&](const void* dptr) { return img + ((const char*)dptr - bt->d_up); };
    u32* h_terms = (u32*)at(bt->d_terms);
    float* h_idf = (float*)at(bt->d_idf);
    u32* h_perm = (u32*)at(bt->d_perm);
    u32* h_grpd = (u32*)at(bt->d_grp);
    bt->weights_ok = bt->k1 >= 0.f && bt->b >= 0.f && bt->b <= 1.f;
    for (size_t i = 0; i < (size_t)B * T && bt->weights_ok; i++) bt->weights_ok = idf[i] >= 0.f && idf[i] <= 3.0e38f;
    const sa_plan pl = sa_batch_plan(bt, true, false);
    sa_batch_order_rows(bt, terms);
    std::vector<u32> h_grp;
    sa_batch_group_rows(bt, terms, idf, pl.group, h_grp);
    for (u32 r = 0; r < B; r++) {
        memcpy(&h_terms[(size_t)r * T], &terms[(size_t)bt->perm[r] * T], T * sizeof(u32));
        memcpy(&h_idf[(size_t)r * T], &idf[(size_t)bt->perm[r] * T], T * sizeof(float));
        h_perm[r] = bt->perm[r];
    }
    {                                                           // minimum-should-match: row r gets the value of caller query perm[r]
        u32* h_mm = (u32*)at(bt->d_min_match);
        for (u32 r = 0; r < B; r++) h_mm[r] = bt->min_match.empty() ? 0u : bt->min_match[bt->perm[r]];
        u32* h_occ = (u32*)at(bt->d_occur);                     // ... and its occur masks (required, prohibited)
        for (u32 r = 0; r < B; r++) {
            h_occ[2 * r] = bt->occur.empty() ? 0u : bt->occur[2 * (size_t)bt->perm[r]];
            h_occ[2 * r + 1] = bt->occur.empty() ? 0u : bt->occur[2 * (size_t)bt->perm[r] + 1];
        }
    }
    memset(h_grpd, 0, (size_t)3 * B * sizeof(u32));
    if (!h_grp.empty()) memcpy(h_grpd, h_grp.data(), h_grp.size() * sizeof(u32));     // (at most B groups)
    memset(at(bt->d_seed), 0, (size_t)B * sizeof(u32));
    if (pl.seed_wanted) sa_impacts_ensure_topf(ix, bt->impacts.get());
    const bool tables = pl.seed_wanted && bt->impacts->d_topf;   // the rank tables and the terms' largest factors exist
    bt->seed_on = tables && !bt->filter && !bt->counting();     // (a filtered, minimum-should-match or occur set starts from 0: the tables' bounds count docs the test may exclude)
    // the staged-tile route's plan (sa_stage.hip): distinct terms, per-query bound tables and the starting bounds, formed on the
    // host into the same upload.  A set that has one does not need the slice table: sa_k_make_bounds is left out of the step and
    // only runs if the run takes another route after all (sa_batch_ensure_bounds)
    bt->stage_ok = false;
    bt->st_dir.reset();
    bt->st_slices.clear();
    // (a filtered set is planned with zero starting bounds: every term staged, none probed)
    if (tables && pl.stage_wanted && !bt->counting()) SA_TRY(sa_stage_plan(bt, img, h_terms, h_idf));
    // the pruning tables: now, if the run will prune (the route rule, now that the groups and the staged plan are known); else on demand
    if (sa_batch_plan(bt, true, false).route == SA_ROUTE_PRUNED) sa_batch_fill_prune_tables(bt, img);
    else { bt->sparse_ok = false; bt->bloom_bytes = 0; bt->sparse_p1_total = 0; bt->sparse_p2_max = 0; }
    const u64 t_host = sa_now_ns();
    SA_TRY(sa_batch_upload_commit(bt));
    bt->bounds_valid = false;
    if (!bt->stage_ok) SA_TRY(sa_batch_ensure_bounds(bt, bt->st));
    SA_HIP(hipGetLastError());
    const u64 t_end = sa_now_ns();
    bt->host_ns[0] += t_host - t_begin; bt->host_ns[1] += t_end - t_host; bt->host_ns[3]++;
    return SA_OK;
}

extern "C" int sa_batch_create(sa_index_t* ix, const uint32_t* terms, const float* idf, int n_queries,
                               int n_query_terms, int k, float k1, float b, sa_batch_t** out) {
    SA_ARG(ix && out && terms && idf, "null argument");
    SA_ARG(n_queries > 0 && n_query_terms > 0, "empty batch");
    SA_ARG(n_query_terms <= SA_MAX_QTERMS, "more than 32 terms per query is not supported");
    SA_ARG(k > 0 && k <= SA_KMAX, "k must be in [1, 1024]");
    SA_ARG(ix->doc_base + ix->n_docs <= 0xFFFFFFFFull, "global doc ids must fit 32 bits for top-k");
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    sa_batch* bt = new (std::nothrow) sa_batch();
    if (!bt) { sa_set_error("out of host memory"); return SA_ERR_NOMEM; }
    bt->opts = sa_options_for_new_handle(&ix->opts);
    bt->ix = ix; bt->B = (u32)n_queries; bt->T = (u32)n_query_terms; bt->k = (u32)k; bt->k1 = k1; bt->b = b;
    int rc = sa_batch_alloc_bm25(bt);
    if (rc == SA_OK) rc = sa_batch_fill(bt, terms, idf);
    if (rc == SA_OK && hipStreamSynchronize(bt->st) != hipSuccess) {
        sa_set_error("sa_batch_create: hipStreamSynchronize failed");
        rc = SA_ERR_HIP;
    }
    if (rc != SA_OK) { sa_batch_free(bt); return rc; }
    *out = bt;
    return SA_OK;
}

// A NEW set of queries in an existing batch (same B, T, k, k1, b): the host derives grouping, pruning tables and
// statistics into a page-locked image, ONE hipMemcpyAsync replaces the device tables and sa_k_make_bounds rebuilds
// the slice table -- all enqueued on the index stream behind the runs still in flight, nothing allocated, nothing
// waited for.  The caller idiom it serves is the reference's score() on a fresh query (postings.py:652-680; timed
// as test/test_msmarco.py:345-395 times it): two batches used alternately keep the device busy while the host
// prepares the next query set.
static int sa_batch_redo_if_flagged(sa_batch* bt);

extern "C" int sa_batch_reset(sa_batch_t* bt, const uint32_t* terms, const float* idf) {
    SA_ARG(bt && bt->ix && terms && idf, "null argument");
    SA_ARG(bt->kind == 0, "sa_batch_reset takes a BM25 batch (phrase batches: sa_phrase_batch_reset)");
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    // a run whose results have not been fetched: its merge (on the exchange stream when sharded) still reads the row order this
    // reset replaces -- wait for that run's result copy first (landed long ago in the run / fetch / reset idiom: no cost there)
    if (bt->res_pending && bt->unfetched) {
        SA_HIP(hipEventSynchronize(bt->ev_res));
        SA_TRY(sa_batch_redo_if_flagged(bt));                   // (a flagged run is redone while the tables still hold ITS query set)
    }
    return sa_batch_fill(bt, terms, idf);
}

// The loaded query set, prepared again for a changed batch state (filter, minimum-should-match): back in caller order from the upload
// image it was filled into (device-row order + the row order; the image's copy to the device has left the host buffer when its event
// has fired; the fill writes the OTHER image).
static int sa_batch_refill(sa_batch* bt) {
    const u32 last = (bt->up_n - 1u) & 1u;
    SA_HIP(hipEventSynchronize(bt->ev_up[last]));
    const char* img = bt->h_up[last];
    const u32* r_terms = (const u32*)(img + ((const char*)bt->d_terms - bt->d_up));
    const float* r_idf = (const float*)(img + ((const char*)bt->d_idf - bt->d_up));
    const size_t T = bt->T;
    std::vector<u32> terms((size_t)bt->B * T);
    std::vector<float> idf((size_t)bt->B * T);
    for (u32 r = 0; r < bt->B; r++) {
        memcpy(&terms[(size_t)bt->perm[r] * T], &r_terms[(size_t)r * T], T * sizeof(u32));
        memcpy(&idf[(size_t)bt->perm[r] * T], &r_idf[(size_t)r * T], T * sizeof(float));
    }
    return sa_batch_fill(bt, terms.data(), idf.data());
}

// Part 2b: the batch ranks inside `f` from its next run on (null: the whole index).  The loaded query set is prepared again -- its
// starting bounds, groups and staged plan belong to the filter state they were made for.
extern "C" int sa_batch_set_filter(sa_batch_t* bt, sa_filter_t* f) {
    SA_ARG(bt && bt->ix, "null batch");
    if (bt->kind != 0) { sa_set_error("sa_batch_set_filter: phrase batches do not take a document filter"); return SA_ERR_UNSUPPORTED; }
    SA_ARG(!f || f->d, "null filter");
    sa_index* ix = bt->ix;
    SA_ARG(!f || (f->d->ix == ix && f->d->n_docs == ix->n_docs), "the filter was built for another index");
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    if (f && sa_opt(bt->opts.no_topk, 0) != 0) { sa_set_error("sa_batch_set_filter: not with the timing option no_topk"); return SA_ERR_UNSUPPORTED; }
    if (!f && !bt->filter) return SA_OK;
    // (as in sa_batch_reset: an unfetched run that was flagged is redone first -- with the filter and the tables it ran with)
    if (bt->res_pending && bt->unfetched) {
        SA_HIP(hipEventSynchronize(bt->ev_res));
        SA_TRY(sa_batch_redo_if_flagged(bt));
    }
    if (bt->filter) SA_HIP(hipStreamSynchronize(bt->st));       // (runs in flight read the bitmap this call may release)
    bt->filter = f ? f->d : nullptr;
    if (sa_opt(bt->opts.trace, 0)) fprintf(stderr, "sa_batch_set_filter: %llu of %llu docs eligible\n", f ? (unsigned long long)f->d->count : (unsigned long long)ix->n_docs, (unsigned long long)ix->n_docs);
    return sa_batch_refill(bt);
}

// Minimum-should-match: from its next run on the batch keeps, for caller query i, only the docs that match at least min_match[i] of
// the query's slots (null: every doc, as before).  The contract of sa_batch_set_filter: the loaded query set is prepared again --
// route, starting bounds, groups and the staged plan belong to the state they were made for -- and the values persist across
// sa_batch_reset / sa_batch_step (row i of every later set gets value i).
extern "C" int sa_batch_set_min_match(sa_batch_t* bt, const uint32_t* min_match) {
    SA_ARG(bt && bt->ix, "null batch");
    if (bt->kind != 0) { sa_set_error("sa_batch_set_min_match: phrase batches do not take minimum-should-match"); return SA_ERR_UNSUPPORTED; }
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    bool on = false;
    for (u32 i = 0; min_match && i < bt->B; i++) on |= min_match[i] > 1u;
    if (on && sa_opt(bt->opts.no_topk, 0) != 0) { sa_set_error("sa_batch_set_min_match: not with the timing option no_topk"); return SA_ERR_UNSUPPORTED; }
    if (on && !sa_min_match_tiles(ix->tile_docs)) {
        sa_set_error("sa_batch_set_min_match: no counting kernel for tile_docs %u (1024, 2048, 4096, 8192)", ix->tile_docs);
        return SA_ERR_UNSUPPORTED;
    }
    if (!min_match && bt->min_match.empty()) return SA_OK;
    // (as in sa_batch_reset: an unfetched run that was flagged is redone first -- with the values and the tables it ran with)
    if (bt->res_pending && bt->unfetched) {
        SA_HIP(hipEventSynchronize(bt->ev_res));
        SA_TRY(sa_batch_redo_if_flagged(bt));
    }
    if (min_match) bt->min_match.assign(min_match, min_match + bt->B);
    else bt->min_match.clear();
    bt->mm_on = on;
    if (sa_opt(bt->opts.trace, 0)) {
        u32 n = 0;
        for (u32 v : bt->min_match) n += v > 1u ? 1u : 0u;
        fprintf(stderr, "sa_batch_set_min_match: %u of %u queries with a value > 1\n", n, bt->B);
    }
    return sa_batch_refill(bt);
}

// Occur classes: from its next run on, slot j of caller query i is optional (0), required (1) or prohibited (2) -- occur[i * T + j];
// null: all optional, as before.  The contract of sa_batch_set_min_match, whose values then count the optional slots.
extern "C" int sa_batch_set_occur(sa_batch_t* bt, const uint8_t* occur) {
    SA_ARG(bt && bt->ix, "null batch");
    if (bt->kind != 0) { sa_set_error("sa_batch_set_occur: phrase batches do not take occur classes"); return SA_ERR_UNSUPPORTED; }
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    const u32 B = bt->B, T = bt->T;                             // (T <= 32, sa_batch_create: a mask has a bit per slot)
    std::vector<u32> masks;
    u32 n_must = 0, n_not = 0;
    if (occur) {
        masks.assign((size_t)2 * B, 0u);
        for (u32 i = 0; i < B; i++)
            for (u32 j = 0; j < T; j++) {
                const uint8_t c = occur[(size_t)i * T + j];
                SA_ARG(c <= 2, "occur classes are 0 (should), 1 (must) and 2 (must_not)");
                if (c) masks[2 * (size_t)i + (c - 1u)] |= 1u << j;
                n_must += c == 1; n_not += c == 2;
            }
    }
    const bool on = n_must + n_not != 0;
    if (on && sa_opt(bt->opts.no_topk, 0) != 0) { sa_set_error("sa_batch_set_occur: not with the timing option no_topk"); return SA_ERR_UNSUPPORTED; }
    if (on && !sa_min_match_tiles(ix->tile_docs)) {
        sa_set_error("sa_batch_set_occur: no counting kernel for tile_docs %u (1024, 2048, 4096, 8192)", ix->tile_docs);
        return SA_ERR_UNSUPPORTED;
    }
    if (!occur && bt->occur.empty()) return SA_OK;
    // (as in sa_batch_reset: an unfetched run that was flagged is redone first -- with the classes and the tables it ran with)
    if (bt->res_pending && bt->unfetched) {
        SA_HIP(hipEventSynchronize(bt->ev_res));
        SA_TRY(sa_batch_redo_if_flagged(bt));
    }
    bt->occur.swap(masks);
    bt->occur_on = on;
    if (sa_opt(bt->opts.trace, 0)) fprintf(stderr, "sa_batch_set_occur: %u required and %u prohibited slots in %u queries\n", n_must, n_not, B);
    return sa_batch_refill(bt);
}

extern "C" int sa_index_set_idf_table(sa_index_t* ix, const float* idf_per_term, uint32_t n_terms) {
    SA_ARG(ix && (idf_per_term || n_terms == 0), "null argument");
    SA_ARG(n_terms == ix->n_terms, "one idf per term of the index");
    // (weights that are negative or not finite keep their batches off the grouped kernel, the starting bounds and the pruning --
    //  every step, silently: the table is checked once, here)
    for (uint32_t t = 0; t < n_terms; t++) SA_ARG(idf_per_term[t] >= 0.f && idf_per_term[t] <= 3.0e38f, "idf table: weights must be finite and >= 0");
    std::lock_guard<std::mutex> g(ix->mu);
    ix->h_idf.assign(idf_per_term, idf_per_term + n_terms);
    return SA_OK;
}


// ---- the shard run (stage 1: tile scoring + per-tile top-k, stage 2: per-shard merge) on the batch's stream

// One launch clears the per-run state of a pruned run -- bound slots / cursors / histograms; only the first run of a batch (or
// the one after a failed run) needs it, every merge leaves the state zeroed -- and, for dynamic pruning, the lead terms' Bloom
// filters.
void sa_batch_clear_state(sa_batch* bt, bool pruned, bool bloom) {
    if (pruned && (!bt->state_clean || bloom)) {
        const size_t words = bt->state_clean ? 0 : (size_t)bt->B * (34 + SA_HBINS);
        const size_t bloom8 = bloom ? bt->bloom_bytes / 8 : 0;            // bloom_bytes is a multiple of 1024
        sa_launch_run_reset(bt->d_slots, (u64)words, bloom ? (u64*)bt->d_bloom : nullptr, (u64)bloom8,
                            bt->state_clean ? nullptr : bt->d_wl_cnt, bt->st);
    }
    bt->state_clean = false;                           // (until this run's merge is enqueued)
}

// The host check of a run that does not defer it: the candidate lists are smaller than the worst case -- did a query run over?
int sa_batch_overflowed(sa_batch* bt, bool* over) {
    std::vector<u32> h_cnt(bt->B);
    SA_HIP(hipMemcpyAsync(h_cnt.data(), bt->d_cand_cnt, (size_t)bt->B * sizeof(u32), hipMemcpyDeviceToHost, bt->st));
    SA_HIP(hipStreamSynchronize(bt->st));
    *over = false;
    for (u32 i = 0; i < bt->B; i++) *over |= h_cnt[i] > bt->cand_cap;
    return SA_OK;
}

// The per-shard merge of the run's candidate lists over n_tiles tiles into shard_out (caller order): append lists of a pruned
// run (bound: the slots, or the histogram bound with `hist`), else [n_tiles][k] blocks.  It leaves the run state zeroed.
void sa_batch_merge_shard(sa_batch* bt, u64* shard_out, u32 n_tiles, bool pruned, bool hist, u32* overflow, const u32* seed) {
    const u32 n_cand = pruned ? bt->cand_cap : (n_tiles ? n_tiles : 1) * bt->k;
    sa_launch_topk_merge(bt->B, bt->st, bt->d_cand, n_cand, bt->k, shard_out, bt->d_perm, 0u, pruned ? bt->d_cand_cnt : nullptr,
                         pruned && !hist ? bt->d_slots : nullptr, pruned && hist ? bt->d_gthr : nullptr, overflow, bt->d_slots, bt->B,
                         1u, bt->d_wl_cnt, 0u, nullptr, seed);
    bt->state_clean = true;
    bt->ran = true;
}

// The tables the planned route reads: the pruning tables if the fill left them out (an option changed since reset: derived
// into the image of the current query set -- once its upload has left the host buffer -- and uploaded again, behind everything
// on this stream), the slice table (every route but the staged one), the Bloom buffer of the pruning route.
static int sa_batch_ensure_tables(sa_batch* bt, const sa_plan& pl) {
    hipStream_t st = bt->st;
    if (pl.route == SA_ROUTE_PRUNED && !bt->sparse_ok) {
        const u32 last = (bt->up_n - 1u) & 1u;
        SA_HIP(hipEventSynchronize(bt->ev_up[last]));
        sa_batch_fill_prune_tables(bt, bt->h_up[last]);
        SA_HIP(hipMemcpyAsync(bt->d_up, bt->h_up[last], bt->up_bytes, hipMemcpyHostToDevice, st));
        SA_HIP(hipEventRecord(bt->ev_up[last], st));
        // (the image carries the starting bounds as the host left them -- zeros: the slice-table kernel forms them again)
        bt->bounds_valid = false;
    }
    if (pl.route != SA_ROUTE_STAGED) SA_TRY(sa_batch_ensure_bounds(bt, st));
    if (pl.route == SA_ROUTE_PRUNED) SA_TRY(sa_batch_ensure_bloom(bt));
    return SA_OK;
}

static Bm25Params sa_batch_params(const sa_batch* bt, const sa_plan& pl) {
    Bm25Params p;
    memset(&p, 0, sizeof(p));
    sa_fill_params(bt->ix, p);
    p.terms = bt->d_terms; p.idf = bt->d_idf; p.B = bt->B; p.T = bt->T; p.k = bt->k;
    p.k1 = bt->k1; p.b = bt->b;
    p.bounds = bt->d_bounds; p.qbase = bt->d_qbase;
    if (pl.imp) {
        p.imp = bt->impacts->d_imp; p.qbase_imp = bt->d_qbase_imp;
        p.imp_tail = bt->impacts->n - 2;
    }
    p.sattab = bt->d_sattab; p.tab_w = bt->tab_w;
    p.pruned = pl.pruned ? 1 : 0;
    p.dense_out = nullptr; p.cand = bt->d_cand;
    p.no_topk = (int)sa_opt(bt->opts.no_topk, 0);
    p.cand_per_tile = bt->k;
    p.cand_cap = bt->cand_cap;
    p.cand_cnt = bt->d_cand_cnt;
    p.slots = bt->d_slots;
    p.hist = pl.hist ? bt->d_hist : nullptr;
    p.gthr = pl.hist ? bt->d_gthr : nullptr;
    p.seed = pl.seed ? bt->d_seed : nullptr;
    p.qlist = nullptr; p.nq = bt->B;
    if (bt->filter) { p.filt = bt->filter->d_words; p.filt_blk = bt->filter->d_blk; p.filt_nblk = bt->filter->n_blocks; }
    if (bt->counting()) { p.min_match_off = (u32)((const char*)bt->d_min_match - (const char*)bt->d_terms); p.stats = bt->d_stats; }     // (sa_batch_stats then counts the (tile, query) items skipped)
    if (bt->occur_on) p.occur_off = (u32)((const char*)bt->d_occur - (const char*)bt->d_terms);
    return p;
}

// The grouped overlay: queries that share their first term -- the first tiles through the per-query kernel, which
// establishes every query's bound (k-th best score so far), then one wave per (tile, group).
// Queries without a group go through the per-query kernel over all tiles.
static int sa_batch_launch_grouped(sa_batch* bt, const Bm25Params& p) {
    sa_index* ix = bt->ix;
    hipStream_t st = bt->st;
    u32 warm = std::max<u32>(16u, bt->k / 8u);     // (k = 1000, 10 M docs: 250 / 128 / 64 warm-up tiles -> 1.07 / 1.02 / 1.05 ms per step)
    // the queries start with bounds from their terms' rank tables (p.seed): no warm-up tiles at all -- the grouped
    // kernel finds bounds above the base values from its first item
    // (10 M docs, k = 10: 16 / 4 / 1 / 0 warm-up tiles 0.394 / 0.396 / 0.388 / 0.383 ms of kernels, without the
    //  starting bounds 0.420; 1.25 M-doc shard: 0.096 / 0.094 / - / 0.0825 against 0.126)
    if (p.seed) warm = 0;
    if (sa_opt_is_set(bt->opts.group_warm)) warm = (u32)std::max<long long>(0, bt->opts.group_warm);
    // a filtered batch warms up on the first tiles that HOLD eligible docs (the tiles in front of them are empty for every kernel):
    // a filter that starts deep in the shard would otherwise leave the overlay without bounds, and every pair to the per-query kernel
    u32 t0 = 0;
    if (bt->filter) t0 = std::min<u32>(bt->filter->first_block / (ix->tile_docs / SA_FILTER_BLOCK), ix->n_tiles);
    warm = std::min(warm, ix->n_tiles - t0);
    // The ungrouped rows (per-query kernel over all tiles) share nothing with the grouped ones -- not a
    // query, not a counter -- so they run on the side stream BESIDE the warm-up tiles and the grouped kernel
    // (a few dense queries are a small grid of long workgroups: alone on the device they took 0.28 ms of a
    // 0.82 ms step on a batch without shared terms); the merge waits for both.
    bool side = false;
    int rc = SA_OK;
    if (bt->n_grouped_rows < bt->B) {
        Bm25Params pu = p;
        pu.qlist = bt->d_iota + bt->n_grouped_rows; pu.nq = bt->B - bt->n_grouped_rows;
        side = true;
        if (!ix->sstream) SA_HIP(hipStreamCreateWithFlags(&ix->sstream, hipStreamNonBlocking));
        for (int i = 0; i < 2; i++)
            if (!bt->ev_side[i]) SA_HIP(hipEventCreateWithFlags(&bt->ev_side[i], hipEventDisableTiming));
        SA_HIP(hipEventRecord(bt->ev_side[0], st));               // (after the reset: the launches above)
        SA_HIP(hipStreamWaitEvent(ix->sstream, bt->ev_side[0], 0));
        rc = sa_launch_bm25(ix, pu, ix->sstream);
        SA_HIP(hipEventRecord(bt->ev_side[1], ix->sstream));
    }
    // (whatever fails from here on, the index stream still joins the side stream: nothing of this run
    //  may be in flight on a stream that sa_batch_free does not wait for in order)
    if (rc == SA_OK) {
        Bm25Params pa = p;
        pa.qlist = bt->d_iota; pa.nq = bt->n_grouped_rows; pa.tile0 = t0; pa.tile_end = t0 + warm;
        rc = sa_launch_bm25(ix, pa, st);
    }
    if (rc == SA_OK && ix->n_tiles > t0 + warm) rc = sa_launch_bm25_groups(ix, bt, p, t0 + warm, st);
    if (side) SA_HIP(hipStreamWaitEvent(st, bt->ev_side[1], 0));
    return rc;
}

static int sa_batch_launch_route(sa_batch* bt, const sa_plan& pl, const Bm25Params& p) {
    sa_index* ix = bt->ix;
    if (ix->avg_doc_len == 0.f || ix->n_tiles == 0) {
        SA_HIP(hipMemsetAsync(bt->d_cand, 0, (size_t)bt->B * p.cand_cap * sizeof(u64), bt->st));
        return SA_OK;
    }
    switch (pl.route) {
        case SA_ROUTE_STAGED: return sa_launch_stage(bt, p, bt->st);
        case SA_ROUTE_PRUNED: {
            // candidates first; a resident grid then scans the queries the sparse path gave back
            SA_TRY(sa_launch_sparse(bt, bt->st));
            Bm25Params pq = p;
            pq.qlist = bt->d_tile_q; pq.nq_dev = bt->d_tile_q + bt->B;
            return sa_launch_bm25_list(ix, pq, bt->st);
        }
        case SA_ROUTE_GROUPED: return sa_batch_launch_grouped(bt, p);
        default: return sa_launch_bm25(ix, p, bt->st);
    }
}

// The shard run of a BM25 batch.  `deferred`: an overflowing candidate list is only flagged on the device (in overflow_cell,
// else d_overflow) and sa_batch_fetch re-runs the batch unpruned before handing out results (no host round trip between the
// tile kernel and the merge); else it is checked here and the batch scored again, unpruned.  `unpruned`: that re-run.
static int sa_batch_run_bm25(sa_batch* bt, u64* shard_out, bool deferred, bool unpruned, u32* overflow_cell) {
    const sa_plan pl = sa_batch_plan(bt, deferred, unpruned);
    SA_TRY(sa_batch_ensure_tables(bt, pl));
    bt->last_route_stage = pl.route == SA_ROUTE_STAGED;
    bt->last_route_sparse = pl.route == SA_ROUTE_PRUNED;
    Bm25Params p = sa_batch_params(bt, pl);
    if (bt->filter && sa_opt(bt->opts.trace, 0))
        fprintf(stderr, "sa_batch: filtered run (%llu of %llu docs eligible): %s\n", (unsigned long long)bt->filter->count, (unsigned long long)bt->ix->n_docs,
                pl.route == SA_ROUTE_STAGED ? "staged tiles" : pl.route == SA_ROUTE_GROUPED ? "grouped overlay + per-query tile kernel" : pl.pruned ? "per-query tile kernel" : "per-query tile kernel, unpruned");
    if (bt->mm_on && sa_opt(bt->opts.trace, 0)) {
        u32 n = 0;
        for (u32 v : bt->min_match) n += v > 1u ? 1u : 0u;
        fprintf(stderr, "sa_batch: minimum-should-match run: %u of %u queries with a value > 1: %s\n", n, bt->B, pl.pruned ? "per-query tile kernel" : "per-query tile kernel, unpruned");
    }
    if (bt->occur_on && sa_opt(bt->opts.trace, 0)) {
        u32 n = 0;
        for (u32 i = 0; i < bt->B; i++) n += (bt->occur[2 * (size_t)i] | bt->occur[2 * (size_t)i + 1]) ? 1u : 0u;
        fprintf(stderr, "sa_batch: occur run: %u of %u queries with a required or prohibited slot: %s\n", n, bt->B, pl.pruned ? "per-query tile kernel" : "per-query tile kernel, unpruned");
    }
    sa_batch_clear_state(bt, pl.pruned, pl.route == SA_ROUTE_PRUNED);
    const u32 slot = bt->ev_n % SA_EVENT_RING;
    SA_HIP(hipEventRecord(bt->ev0[slot], bt->st));
    SA_TRY(sa_batch_launch_route(bt, pl, p));
    SA_HIP(hipEventRecord(bt->ev1[slot], bt->st));
    bt->ev_n++;
    if (pl.may_overflow && !deferred) {
        bool over = false;
        SA_TRY(sa_batch_overflowed(bt, &over));
        if (over) {
            p.pruned = 0; p.hist = nullptr; p.gthr = nullptr;
            SA_TRY(sa_launch_bm25(bt->ix, p, bt->st));
        }
    }
    sa_batch_merge_shard(bt, shard_out, bt->ix->n_tiles, p.pruned != 0, p.hist != nullptr,
                         pl.may_overflow && deferred ? (overflow_cell ? overflow_cell : bt->d_overflow) : nullptr, p.seed);
    return SA_OK;
}

// stage 3: merge the per-rank top-k lists [nranks][B*k (+ extra)] (device memory) into d_final
static int sa_batch_merge_ranks(sa_batch* bt, const u64* d_gathered, int nranks, hipStream_t st, u32 extra = 0) {
    const size_t count = (size_t)bt->B * bt->k;
    if ((u64)nranks * bt->k <= (u64)SA_MERGE_LIST) {
        // the usual case: the gathered keys of a query fit the merge's LDS list -- one launch reads them where they are
        sa_launch_topk_merge(bt->B, st, (u64*)d_gathered, (u32)nranks * bt->k, bt->k, bt->d_final, nullptr, bt->k, nullptr, nullptr,
                             nullptr, nullptr, nullptr, 0u, 0u, nullptr, (u32)(count + extra), extra ? bt->d_xflag : nullptr, nullptr);
        return SA_OK;
    }
    if (!bt->d_xcand || bt->xcand_ranks < nranks) {
        if (bt->d_xcand) SA_HIP(hipFree(bt->d_xcand));
        bt->d_xcand = nullptr;
        SA_HIP(hipMalloc(&bt->d_xcand, (size_t)nranks * count * sizeof(u64)));
        bt->xcand_ranks = nranks;
    }
    sa_launch_regroup(d_gathered, (u32)nranks, bt->B, bt->k, extra, bt->d_xcand, bt->d_xflag, st);
    // every rank's block is its sorted top-k: group leaders = rank maxima
    sa_launch_topk_merge(bt->B, st, bt->d_xcand, (u32)nranks * bt->k, bt->k, bt->d_final, nullptr, bt->k, nullptr, nullptr, nullptr,
                         nullptr, nullptr, 0u, 0u, nullptr, 0u, nullptr, nullptr);
    return SA_OK;
}

// A run whose result copy has landed (bt->h_res): was it flagged?  1: a candidate list overflowed (only possible when the
// bound could not rise: degenerate score distributions); 2: fewer than k keys at or above a bound (a starting bound was too
// high).  The batch is then REDONE with the unpruned selection -- against the device tables of the query set that run scored,
// which is why sa_batch_reset / sa_batch_step call this for a run nobody has fetched yet BEFORE they replace those tables
// (round 4 redid at fetch time only: a flagged run followed by reset + fetch returned the new set's results as the old set's).
// Sharded: every rank saw the same flag (it travelled with the all-gather) and every rank makes the same calls, so all of
// them redo the exchange.  Only BM25 runs are ever flagged (a phrase run checks overflow on the host and has no starting
// bounds).  Call with the index lock held, after ev_res has fired.
static int sa_batch_redo_if_flagged(sa_batch* bt) {
    sa_index* ix = bt->ix;
    const size_t n = (size_t)bt->B * bt->k;
    const u32 over = (u32)bt->h_res[n + (ix->comm ? 1 : 0)];
    if (!over) return SA_OK;
    if (sa_opt(bt->opts.trace, 0)) fprintf(stderr, "sa_batch: run redone without bounds (flag %u)\n", over);
    SA_HIP(hipStreamSynchronize(bt->st));
    if (ix->xstream) SA_HIP(hipStreamSynchronize(ix->xstream));
    SA_HIP(hipMemset(bt->d_overflow, 0, sizeof(u32)));
    SA_HIP(hipMemset(bt->d_xflag, 0, sizeof(u32)));
    if (bt->d_xlocal) {
        SA_HIP(hipMemset(bt->d_xlocal + n, 0, sizeof(u64)));
        SA_HIP(hipMemset(bt->d_xlocal + 2 * n + 1, 0, sizeof(u64)));
    }
    if (ix->comm) {
        const size_t count = n;
        int nranks = 1;
        SA_TRY(sa_comm_allgather_topk(ix, nullptr, nullptr, 0, &nranks, ix->xstream));
        SA_TRY(sa_batch_run_bm25(bt, bt->d_xlocal, false, true, nullptr));
        SA_HIP(hipStreamSynchronize(bt->st));
        SA_TRY(sa_comm_allgather_topk(ix, bt->d_xlocal, bt->d_gather, count, &nranks, ix->xstream));
        SA_TRY(sa_batch_merge_ranks(bt, bt->d_gather, nranks, ix->xstream));
        SA_HIP(hipStreamSynchronize(ix->xstream));
    } else {
        SA_TRY(sa_batch_run_bm25(bt, bt->d_final, false, true, nullptr));
        SA_HIP(hipStreamSynchronize(bt->st));
    }
    SA_HIP(hipGetLastError());
    SA_HIP(hipMemcpy(bt->h_res, bt->d_final, (n + 2) * sizeof(u64), hipMemcpyDeviceToHost));
    bt->h_res[n] = 0; bt->h_res[n + 1] = 0;                     // (the image now holds the redone results: nothing left to flag)
    return SA_OK;
}

// Results to the host without synchronising a stream: the keys and the two overflow flags behind them are copied into
// the batch's page-locked result buffer and sa_batch_fetch waits for the copy's event only.  ALL result copies of an
// index go through its one exchange stream, behind an event of the stream that wrote the keys: device-to-host copies
// issued on the batches' own streams hold those streams up -- measured with 4 batches in flight on a 1.25 M-doc shard:
// 0.200 ms per step with the copies on the batch streams, 0.113 ms on the exchange stream.
static int sa_batch_queue_result_copy(sa_batch* bt, hipStream_t src_stream) {
    const size_t n = (size_t)bt->B * bt->k + 2;
    sa_index* ix = bt->ix;
    if (!ix->xstream) SA_HIP(hipStreamCreateWithFlags(&ix->xstream, hipStreamNonBlocking));
    if (src_stream != ix->xstream) {
        SA_HIP(hipEventRecord(bt->ev_final, src_stream));
        SA_HIP(hipStreamWaitEvent(ix->xstream, bt->ev_final, 0));
    }
    SA_HIP(hipMemcpyAsync(bt->h_res, bt->d_final, n * sizeof(u64), hipMemcpyDeviceToHost, ix->xstream));
    SA_HIP(hipEventRecord(bt->ev_res, ix->xstream));
    bt->res_pending = true;
    bt->unfetched = true;
    return SA_OK;
}

// sa_batch_run with the index lock held (sa_batch_step fills and runs under ONE lock: no other thread's call on the batch
// or the index lands between the two)
static int sa_batch_run_locked(sa_batch* bt, int sync, sa_shard_run run_shard) {
    sa_index* ix = bt->ix;
    SA_HIP(hipSetDevice(ix->device));
    hipStream_t st = bt->st;
    const u64 t_run = sa_now_ns();
    struct RunClock { sa_batch* b; u64 t0; ~RunClock() { b->host_ns[2] += sa_now_ns() - t0; } } run_clock{bt, t_run};
    if (ix->comm) {
        // Scoring runs on the index stream; the all-gather of the per-shard top-k and the
        // cross-rank merge run on the exchange stream, double-buffered, so they overlap the next
        // run's scoring kernels (the exchange is latency-bound: B*k*8 bytes per rank).  Every rank's block ends
        // with one extra cell, its overflow flag: the ranks learn from the exchange itself whether any of them
        // has to redo the batch unpruned (sa_batch_fetch) -- no separate collective, no host round trip.
        int nranks = 1;
        const size_t count = (size_t)bt->B * bt->k;
        const size_t cell = count + 1;
        hipStream_t xs = ix->xstream;
        SA_TRY(sa_comm_allgather_topk(ix, nullptr, nullptr, 0, &nranks, xs));
        if (!bt->d_xlocal) {
            SA_HIP(hipMalloc(&bt->d_xlocal, 2 * cell * sizeof(u64)));
            SA_HIP(hipMemset(bt->d_xlocal, 0, 2 * cell * sizeof(u64)));
            for (int i = 0; i < 2; i++) {
                SA_HIP(hipEventCreateWithFlags(&bt->ev_scored[i], hipEventDisableTiming));
                SA_HIP(hipEventCreateWithFlags(&bt->ev_exchanged[i], hipEventDisableTiming));
            }
        }
        if (!bt->d_gather || bt->gather_ranks < nranks) {
            SA_HIP(hipStreamSynchronize(xs));
            if (bt->d_gather) SA_HIP(hipFree(bt->d_gather));
            bt->d_gather = nullptr;
            SA_HIP(hipMalloc(&bt->d_gather, 2 * (size_t)nranks * cell * sizeof(u64)));
            bt->gather_ranks = nranks;
        }
        if ((u64)nranks * bt->k > (u64)SA_MERGE_LIST && (!bt->d_xcand || bt->xcand_ranks < nranks))
            SA_HIP(hipStreamSynchronize(xs));                                             // merge_ranks reallocates
        const u32 bsel = bt->xstep & 1;
        bt->xstep++;
        u64* xl = bt->d_xlocal + bsel * cell;
        u64* xg = bt->d_gather + bsel * (size_t)nranks * cell;
        if (bt->exchanged_valid[bsel]) SA_HIP(hipStreamWaitEvent(st, bt->ev_exchanged[bsel], 0));
        SA_TRY(run_shard(bt, xl, true, false, (u32*)(xl + count)));      // (the flag cell: set by the shard merge, sticky until fetch)
        SA_HIP(hipEventRecord(bt->ev_scored[bsel], st));
        SA_HIP(hipStreamWaitEvent(xs, bt->ev_scored[bsel], 0));
        SA_TRY(sa_comm_allgather_topk(ix, xl, xg, cell, &nranks, xs));
        SA_TRY(sa_batch_merge_ranks(bt, xg, nranks, xs, 1u));
        SA_TRY(sa_batch_queue_result_copy(bt, xs));
        SA_HIP(hipEventRecord(bt->ev_exchanged[bsel], xs));
        bt->exchanged_valid[bsel] = true;
        if (sync) SA_HIP(hipStreamSynchronize(xs));
    } else {
        SA_TRY(run_shard(bt, bt->d_final, true, false, nullptr));
        SA_TRY(sa_batch_queue_result_copy(bt, st));
    }
    if (sync) {
        SA_HIP(hipStreamSynchronize(st));
        SA_HIP(hipGetLastError());
    }
    return SA_OK;
}

extern "C" int sa_batch_run(sa_batch_t* bt, int sync) {
    SA_ARG(bt && bt->ix, "null batch");
    std::lock_guard<std::mutex> g(bt->ix->mu);
    return sa_batch_run_locked(bt, sync, bt->kind == 1 ? sa_phrase_batch_run_shard : sa_batch_run_bm25);
}

// One step of a query stream in one call: idf gathered from the index's table, reset, run (header, Part 2) -- under one lock.
extern "C" int sa_batch_step(sa_batch_t* bt, const uint32_t* terms) {
    SA_ARG(bt && bt->ix && terms, "null argument");
    SA_ARG(bt->kind == 0, "sa_batch_step takes a BM25 batch");
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_ARG(ix->h_idf.size() == ix->n_terms, "sa_index_set_idf_table has not been called");
    SA_HIP(hipSetDevice(ix->device));
    const size_t n = (size_t)bt->B * bt->T;
    bt->step_idf.resize(n);
    for (size_t i = 0; i < n; i++) bt->step_idf[i] = terms[i] < ix->n_terms ? ix->h_idf[terms[i]] : 0.f;
    if (bt->res_pending && bt->unfetched) {
        SA_HIP(hipEventSynchronize(bt->ev_res));
        SA_TRY(sa_batch_redo_if_flagged(bt));                   // (a flagged run is redone while the tables still hold ITS query set)
    }
    SA_TRY(sa_batch_fill(bt, terms, bt->step_idf.data()));
    return sa_batch_run_locked(bt, 0, sa_batch_run_bm25);
}

extern "C" int sa_batch_seeds(sa_batch_t* bt, float* out) {
    SA_ARG(bt && bt->ix && out, "null argument");
    SA_ARG(bt->kind == 0, "sa_batch_seeds takes a BM25 batch");
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    SA_HIP(hipStreamSynchronize(bt->st));
    std::vector<u32> rows(bt->B);
    SA_HIP(hipMemcpy(rows.data(), bt->d_seed, (size_t)bt->B * sizeof(u32), hipMemcpyDeviceToHost));
    for (u32 r = 0; r < bt->B; r++) {                           // device row r holds caller query perm[r]
        float f;
        memcpy(&f, &rows[r], 4);
        out[bt->perm[r]] = bt->seed_on ? f : 0.f;
    }
    return SA_OK;
}

extern "C" int sa_batch_host_times(sa_batch_t* bt, uint64_t* out4) {
    SA_ARG(bt && out4, "null argument");
    for (int i = 0; i < 4; i++) out4[i] = bt->host_ns[i];
    return SA_OK;
}

// External-collective variant (the caller owns the exchange, e.g. torch.distributed over RCCL,
// or gloo in the CPU tests): run this shard, hand out its top-k keys, merge gathered keys.
extern "C" int sa_batch_run_local(sa_batch_t* bt, void* local_keys_out_device, int sync) {
    SA_ARG(bt && bt->ix, "null batch");
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    bt->res_pending = false;                           // (the external-collective route: fetch reads d_final, not the page-locked copy of an earlier sa_batch_run)
    SA_TRY((bt->kind == 1 ? sa_phrase_batch_run_shard : sa_batch_run_bm25)(bt, bt->d_local, false, false, nullptr));
    if (local_keys_out_device)
        SA_HIP(hipMemcpyAsync(local_keys_out_device, bt->d_local, (size_t)bt->B * bt->k * sizeof(u64),
                              hipMemcpyDefault, bt->st));      // (the caller's buffer: device memory, or page-locked host memory)
    if (sync) {
        SA_HIP(hipStreamSynchronize(bt->st));
        SA_HIP(hipGetLastError());
    }
    return SA_OK;
}

extern "C" int sa_batch_merge_gathered(sa_batch_t* bt, const void* gathered_keys_device, int nranks, int sync) {
    SA_ARG(bt && bt->ix && gathered_keys_device, "null argument");
    SA_ARG(nranks >= 1, "nranks < 1");
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    bt->res_pending = false;
    SA_TRY(sa_batch_merge_ranks(bt, (const u64*)gathered_keys_device, nranks, bt->st));
    if (sync) {
        SA_HIP(hipStreamSynchronize(bt->st));
        SA_HIP(hipGetLastError());
    }
    return SA_OK;
}

extern "C" int sa_batch_fetch(sa_batch_t* bt, float* scores_out, uint64_t* docs_out) {
    SA_ARG(bt && bt->ix && scores_out && docs_out, "null argument");
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    const size_t n = (size_t)bt->B * bt->k;
    const u64* keys = nullptr;
    std::vector<u64> legacy;
    if (bt->res_pending) {
        // the usual route (sa_batch_run): wait for THIS batch's result copy, nothing else -- other batches of the
        // index may be in flight behind it
        SA_HIP(hipEventSynchronize(bt->ev_res));
        bt->unfetched = false;
        SA_TRY(sa_batch_redo_if_flagged(bt));
        keys = bt->h_res;
    } else {
        // external-collective route (sa_batch_run_local / sa_batch_merge_gathered): the caller's last call decides
        legacy.resize(n);
        SA_HIP(hipStreamSynchronize(bt->st));
        if (ix->xstream) SA_HIP(hipStreamSynchronize(ix->xstream));
        SA_HIP(hipGetLastError());
        SA_HIP(hipMemcpy(legacy.data(), bt->d_final, n * sizeof(u64), hipMemcpyDeviceToHost));
        keys = legacy.data();
    }
    for (u32 r = 0; r < bt->B; r++) {
        const u32 qi = r;                        // results are stored in caller order
        for (u32 j = 0; j < bt->k; j++) {
            const u64 key = keys[(size_t)r * bt->k + j];
            const u32 sb = (u32)(key >> 32);
            float s;
            memcpy(&s, &sb, 4);
            scores_out[(size_t)qi * bt->k + j] = key ? s : 0.f;
            docs_out[(size_t)qi * bt->k + j] = key ? (u64)(u32)(~(u32)(key & 0xFFFFFFFFull)) : SA_NO_DOC;
        }
    }
    return SA_OK;
}

// Part 2d: hit counts and facet counts of the loaded query set under the batch's current filter / minimum-should-match / occur state
// (header).  One launch of the facet kernel (sa_k_bm25_facet_tiles, sa_bm25.hip) on the batch's stream, behind whatever is in flight:
// the parameters of an unpruned run over the TF postings -- no impact stream, no bounds, no candidates --, so the matched set is the one
// a run with k = n_docs would rank.  It reads the slice table (built here if the last fill left it to the staged route: the same launch
// sa_batch_ensure_tables makes when a run changes route) and the saturation table (built with the batch), and writes its own counters
// only: the run state, the candidate lists and the results of a run nobody has fetched stay as they are.
extern "C" int sa_batch_facet_counts(sa_batch_t* bt, sa_codes_t* codes, uint64_t* found_out, uint64_t* missing_out, uint32_t* counts_out) {
    SA_ARG(bt && bt->ix && found_out, "null argument");
    if (bt->kind != 0) { sa_set_error("sa_batch_facet_counts: phrase batches have no facet counts"); return SA_ERR_UNSUPPORTED; }
    sa_index* ix = bt->ix;
    if (!sa_min_match_tiles(ix->tile_docs)) {
        sa_set_error("sa_batch_facet_counts: no counting kernel for tile_docs %u (1024, 2048, 4096, 8192)", ix->tile_docs);
        return SA_ERR_UNSUPPORTED;
    }
    const size_t B = bt->B;
    const size_t V = codes ? codes->n_values : 0;
    if (codes) {
        SA_ARG(missing_out && counts_out, "missing_out / counts_out null with a column");
        SA_ARG(codes->d || codes->n_docs == 0, "null column");
        SA_ARG(codes->device == ix->device, "the column lives on another device than the batch");
        SA_ARG(codes->n_docs == ix->n_docs, "the column covers another number of documents than the index holds");
        SA_ARG((u64)B * V <= SA_FACET_MAX_CELLS, "queries x values of one call must not exceed 2^28");
    }
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    for (size_t i = 0; i < B; i++) found_out[i] = 0;
    if (codes) {
        for (size_t i = 0; i < B; i++) missing_out[i] = 0;
        memset(counts_out, 0, B * V * sizeof(u32));
    }
    // (as sa_batch_launch_route: nothing scores in an empty shard or with an average doc length of 0)
    if (ix->n_tiles == 0 || ix->n_docs == 0 || ix->avg_doc_len == 0.f) return SA_OK;
    hipStream_t st = bt->st;
    const size_t words = 2 * B + B * V;
    if (bt->facet_words < words) {
        if (bt->d_facet) {                                      // (no call is in flight: every call waits for its own work)
            SA_HIP(hipFree(bt->d_facet));
            bt->d_facet = nullptr; bt->facet_words = 0;
        }
        SA_HIP(hipMalloc(&bt->d_facet, words * sizeof(u32)));
        bt->facet_words = words;
    }
    SA_TRY(sa_batch_ensure_bounds(bt, st));
    const sa_plan pl{};                                     // unpruned, not impact, not seeded: MODE 0 over the TF postings
    Bm25Params p = sa_batch_params(bt, pl);
    p.cand = nullptr; p.dense_out = nullptr; p.stats = nullptr; p.no_topk = 0;
    // (a filtered batch: the tiles in front of the filter's first eligible block are empty for every item)
    if (bt->filter) p.tile0 = std::min<u32>(bt->filter->first_block / (ix->tile_docs / SA_FILTER_BLOCK), ix->n_tiles);
    FacetParams fp;
    fp.codes = codes ? codes->d : nullptr;
    fp.n_values = (u32)V;
    fp.found = bt->d_facet; fp.missing = bt->d_facet + B; fp.counts = bt->d_facet + 2 * B;
    fp.row = bt->d_perm;
    SA_HIP(hipMemsetAsync(bt->d_facet, 0, words * sizeof(u32), st));
    SA_TRY(sa_launch_bm25_facet(ix, p, fp, st));
    SA_HIP(hipGetLastError());
    std::vector<u32> h(2 * B);
    SA_HIP(hipMemcpyAsync(h.data(), bt->d_facet, 2 * B * sizeof(u32), hipMemcpyDeviceToHost, st));
    if (codes && V) SA_HIP(hipMemcpyAsync(counts_out, fp.counts, B * V * sizeof(u32), hipMemcpyDeviceToHost, st));
    SA_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < B; i++) {
        found_out[i] = h[i];
        if (codes) missing_out[i] = h[B + i];
    }
    return SA_OK;
}

// Diagnostics: switch on per-query counting of the candidate docs the sparse path scores (an extra
// atomic per candidate, so not for timed runs) and read the totals of the runs since the previous call.
extern "C" int sa_batch_stats(sa_batch_t* bt, int enable, uint64_t* sparse_candidates_out, uint64_t* sparse_queries_out) {
    SA_ARG(bt && bt->ix, "null batch");
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    SA_HIP(hipStreamSynchronize(bt->st));
    u64 total = 0, nq = 0;
    if (bt->d_stats) {
        std::vector<u32> h(bt->B);
        SA_HIP(hipMemcpy(h.data(), bt->d_stats, (size_t)bt->B * sizeof(u32), hipMemcpyDeviceToHost));
        for (u32 v : h) total += v;
        SA_HIP(hipMemset(bt->d_stats, 0, (size_t)bt->B * sizeof(u32)));
    }
    if (bt->d_route) {
        std::vector<u32> h(bt->B);
        SA_HIP(hipMemcpy(h.data(), bt->d_route, (size_t)bt->B * sizeof(u32), hipMemcpyDeviceToHost));
        for (u32 v : h) nq += v == 0 ? 1 : 0;
    }
    if (enable && !bt->d_stats) {
        SA_HIP(hipMalloc(&bt->d_stats, (size_t)bt->B * sizeof(u32)));
        SA_HIP(hipMemset(bt->d_stats, 0, (size_t)bt->B * sizeof(u32)));
    } else if (!enable && bt->d_stats) {
        SA_HIP(hipFree(bt->d_stats));
        bt->d_stats = nullptr;
    }
    if (sparse_candidates_out) *sparse_candidates_out = total;
    if (sparse_queries_out) *sparse_queries_out = nq;
    return SA_OK;
}

extern "C" int sa_batch_profile(sa_batch_t* bt, double* kernel_ms_out, uint64_t* alg_bytes_out,
                                uint64_t* postings_bytes_out) {
    SA_ARG(bt && bt->ix, "null batch");
    SA_ARG(bt->ran && bt->ev_n > 0, "batch has not been run since the last profile call");
    sa_index* ix = bt->ix;
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    SA_HIP(hipStreamSynchronize(bt->st));
    // mean over the runs since the previous call (at most the last SA_EVENT_RING of them)
    const u32 n = bt->ev_n < SA_EVENT_RING ? bt->ev_n : SA_EVENT_RING;
    double sum = 0.0;
    for (u32 i = 0; i < n; i++) {
        float ms = 0.f;
        SA_HIP(hipEventElapsedTime(&ms, bt->ev0[i], bt->ev1[i]));
        sum += ms;
    }
    bt->ev_n = 0;
    if (kernel_ms_out) *kernel_ms_out = n ? sum / n : 0.0;
    if (alg_bytes_out) *alg_bytes_out = bt->alg_bytes;
    if (postings_bytes_out) *postings_bytes_out = bt->postings_bytes;
    return SA_OK;
}

extern "C" int sa_batch_last_route(sa_batch_t* bt, int* pruned_out) {
    SA_ARG(bt && bt->ix && pruned_out, "null argument");
    std::lock_guard<std::mutex> g(bt->ix->mu);
    *pruned_out = bt->last_route_stage ? 2 : bt->last_route_sparse ? 1 : 0;
    return SA_OK;
}

// Diagnostics: the caller query that each device row of the current set holds (row r -> out[r]); tests check that per-query tables
// written through this order (sa_batch_set_min_match) are exercised with an order that is not the identity.
extern "C" int sa_batch_row_order(sa_batch_t* bt, uint32_t* out) {
    SA_ARG(bt && bt->ix && out, "null argument");
    SA_ARG(bt->kind == 0, "sa_batch_row_order takes a BM25 batch");
    std::lock_guard<std::mutex> g(bt->ix->mu);
    for (u32 r = 0; r < bt->B; r++) out[r] = bt->perm[r];
    return SA_OK;
}

extern "C" int sa_batch_group_info(sa_batch_t* bt, uint32_t out[4]) {
    SA_ARG(bt && out, "null argument");
    out[0] = bt->n_groups; out[1] = bt->n_grouped_rows; out[2] = bt->n_shared_rows; out[3] = bt->B - bt->n_grouped_rows;
    return SA_OK;
}

// A batch's switches after its creation: effective from its next reset / run (what was sized at creation -- candidate
// capacity, streams, the phrase tile size -- keeps what it was).
extern "C" int sa_batch_set_options(sa_batch_t* bt, const sa_options_t* o) {
    SA_ARG(bt && bt->ix && o, "null argument");
    SA_ARG(o->struct_size == sizeof(sa_options_t), "sa_options_t: wrong struct_size (fill it with sa_options_init)");
    std::lock_guard<std::mutex> g(bt->ix->mu);
    bt->opts = *o;
    return SA_OK;
}
extern "C" int sa_batch_get_options(sa_batch_t* bt, sa_options_t* out) {
    SA_ARG(bt && bt->ix && out, "null argument");
    std::lock_guard<std::mutex> g(bt->ix->mu);
    *out = bt->opts;
    return SA_OK;
}

// Diagnostics: the rank table of a term in this batch's impact stream (22 lower bounds of its r-th largest factor, sa_topf_ranks) and its
// exact largest factor -- what the starting bounds are formed from.  Tests compare the tables of differently built streams.
extern "C" int sa_batch_debug_rank_table(sa_batch_t* bt, uint32_t term, float* ranks22_out, float* maxf_out) {
    SA_ARG(bt && bt->ix && ranks22_out && maxf_out, "null argument");
    std::lock_guard<std::mutex> g(bt->ix->mu);
    sa_impacts* im = bt->impacts.get();
    if (!im || term >= bt->ix->n_terms || im->h_topf.size() != (size_t)bt->ix->n_terms * SA_TOPF_NR || im->h_maxf.size() != bt->ix->n_terms) {
        sa_set_error("sa_batch_debug_rank_table: the batch has no rank tables (no impact stream, term_seed = 0, or an unknown term)");
        return SA_ERR_STATE;
    }
    memcpy(ranks22_out, &im->h_topf[(size_t)term * SA_TOPF_NR], SA_TOPF_NR * sizeof(float));
    *maxf_out = im->h_maxf[term];
    return SA_OK;
}

extern "C" int sa_batch_destroy(sa_batch_t* bt) {
    if (!bt) return SA_OK;
    // (under the index lock: a dense call on another thread swaps ix->stream / scratch to its lane while it holds the lock --
    //  sa_batch_free must synchronise the index's own stream, not a lane's)
    if (bt->ix) { std::lock_guard<std::mutex> g(bt->ix->mu); sa_batch_free(bt); }
    else sa_batch_free(bt);
    return SA_OK;
}
