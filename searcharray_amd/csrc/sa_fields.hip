// sa_fields.hip -- Part 4b of the C ABI: a batch of MULTI-FIELD (Solr edismax, term-centric) queries ranked in one pass.
//
// What searcharray_amd.solr.edismax_search does per query -- T x F dense float32[n_docs] score vectors, T x (F + 1) element-wise
// float64 passes over [n_docs] (sa_vec.hip: sa_vec_dismax_acc / sa_vec_clause / sa_vec_mask_min_count) and a radix select
// (sa_vec_topk.hip) -- is formed here per (tile, query) item in LDS, straight from the fields' impact streams.  No [n_docs] vector is
// written for any query; per query k (score, row) pairs and one count leave the device.
//
// ARITHMETIC (why the result is bit-identical to the per-query route).  For clause t and field f the value of a posting is
//     s = fl32(factor x w[t][f])  ( x boost[f] when the field has one)
// -- what sa_k_bm25_dense_direct stores for a one-term call (its accumulator starts at +0: 0 + s == s) and sa_index_bm25_dense_to scales.
// Per doc, fields in qf order:   sum = fl64(sum + (double)s) ;  mx = max(mx, (double)s)           (sa_k_vec_dismax_acc)
// after the clause's last field: c = fl64(mx + fl64(fl64(sum - mx) x tie)) ; total = fl64(total + c) ; cnt += c > 0   (sa_k_vec_clause)
// after the last clause:         total = 0 where cnt < need                                                   (sa_k_vec_mask64)
// A doc that a field's term does not hold gets s = +0.0 on the vector route: sum + 0.0 and max(mx, 0.0) leave the bits as they are
// (sum and mx start at +0.0 and never go below it), so skipping the doc is the same operation.  mx only ever holds float32 values,
// so it is kept as a float; a clause no field has postings for in the tile gives c = +0.0 for every doc and is skipped.  Every
// operation is an explicit round-to-nearest intrinsic: no contraction, no reassociation.
//
// SCORE KERNEL (sa_k_fields_score<TILE>, 256 threads, one workgroup per (tile, query) item, query fastest).  LDS per doc: sum f64,
// total f64, mx f32, cnt u8 = 21 bytes -> 21.5 / 43 / 86 KB for tiles of 1024 / 2048 / 4096 docs (+ 3.1 KB of slice table and
// reduction scratch): 6 / 3 / 1 workgroups per CU of the 160 KiB.  A (clause, field) slice is found like sa_k_bm25_dense_direct's: the
// field's tile directory row when the term has one AND the field's index was built for this tile size, else two searches of the
// term's TF postings.  Within one (clause, field) pass a doc occurs at most once (a term holds a doc once), so lanes never meet on an
// accumulator; a barrier separates the passes.  An item whose filter blocks are empty, or that has no posting in the tile, writes its
// count 0 and nothing else.  Selection: the doubles are positive, so their bit patterns order as u64 (sa_block_kth_largest on the
// patterns); entries above the threshold are all taken, entries equal to it by lowest doc first (a block scan in doc order).
//
// MERGE KERNEL (sa_k_fields_merge, one workgroup per query): streams the query's candidate slots, keeps the best in a sorted LDS
// buffer and appends only candidates that beat the current k-th entry to a pending region; the buffer is re-sorted (bitonic, pair
// comparison: bits descending, doc ascending) when the pending region could overflow and at the end.  Exact for any number of
// candidates; the result does not depend on the order in which candidates are appended (the sort erases it).
#include "sa_batch.hpp"
#include "sa_bm25_params.hpp"
#include "sa_filter.hpp"
#include "../../include/searcharray_hip.h"
#include <algorithm>
#include <new>

#define SA_FB_MAXF 8
#define SA_FB_THREADS 256
#define SA_FB_MERGE_LIST 4096u                   // pairs of one query the merge holds in LDS (48 KB): the best (up to 1024) + the pending region.
                                                 // (with 2048 the region of a k = 1000 merge was one round of 1024 candidates: a sort per round, 20 ms
                                                 //  for 256 queries x 245 tiles)
#define SA_FB_DEFAULT_CAND_MB 256                // option fields_cand_mb: candidate scratch of a batch at most (queries run in slices)

struct FieldsParams {
    // the fields
    const u64* tfp[SA_FB_MAXF];
    const u64* tf_off[SA_FB_MAXF];
    const u32* dir_slot[SA_FB_MAXF];             // null: the field's index has another tile size (search the postings)
    const u32* tile_dir[SA_FB_MAXF];
    const u64* imp[SA_FB_MAXF];                  // null: the field contributes zeros (no postings, or avg_doc_len == 0)
    u32 n_terms[SA_FB_MAXF];
    float boost[SA_FB_MAXF];
    int has_boost[SA_FB_MAXF];
    u32 F, T, n_tiles, k, kk;                    // kk = min(k, TILE): candidates an item keeps
    u64 n_docs;
    double tie;
    // the query set (device, whole batch) and the slice [q0, q0 + nq) this launch scores
    const u32* terms;                            // [B][T][F]
    const float* w;                              // [B][T][F]
    const u32* need;                             // [B]
    u32 q0, nq;
    // filter (null: none)
    const u32* fwords;
    const u32* fblk;
    u32 n_fblocks;
    // out
    u64* cand_bits;                              // [nq][n_tiles][kk]
    u32* cand_doc;                               // [nq][n_tiles][kk]
    u32* item_cnt;                               // [nq][n_tiles]
    unsigned long long* found;                   // [B]
};

__device__ __forceinline__ u64 sa_f64_bits(double d) { u64 u; __builtin_memcpy(&u, &d, 8); return u; }

template <int TILE>
__global__ void __launch_bounds__(SA_FB_THREADS) sa_k_fields_score(const FieldsParams p) {
    constexpr int E = TILE / SA_FB_THREADS;
    constexpr int NW = SA_FB_THREADS / SA_WAVE;
    __shared__ double s_sum[TILE];
    __shared__ double s_total[TILE];
    __shared__ float s_mx[TILE];
    __shared__ unsigned char s_cnt[TILE];
    __shared__ u64 s_first[SA_FB_THREADS];
    __shared__ u32 s_n[SA_FB_THREADS];
    __shared__ u64 red64[NW];
    __shared__ u32 red[NW + 1];
    const u32 tid = threadIdx.x;
    const u32 ql = blockIdx.x % p.nq, tile = blockIdx.x / p.nq;       // (query fastest: the items of a tile run together)
    const u32 q = p.q0 + ql;
    const u64 oi = (u64)ql * p.n_tiles + tile;
    const u64 d0 = (u64)tile * TILE;
    if (p.fblk) {                                                     // (workgroup-uniform) no eligible doc in the tile: nothing is read
        u32 any = 0;
        for (u32 i = 0; i < (u32)TILE / SA_FILTER_BLOCK; i++) {
            const u32 blk = tile * ((u32)TILE / SA_FILTER_BLOCK) + i;
            if (blk < p.n_fblocks) any |= p.fblk[blk];
        }
        if (any == 0) { if (tid == 0) p.item_cnt[oi] = 0; return; }
    }
#pragma unroll
    for (int j = 0; j < E; j++) {
        const u32 e = (u32)j * SA_FB_THREADS + tid;
        s_sum[e] = 0.0; s_total[e] = 0.0; s_mx[e] = 0.f; s_cnt[e] = 0;
    }
    // the tile's slice of every (clause, field) term
    const u32 TF = p.T * p.F;
    u64 first = 0; u32 n = 0;
    if (tid < TF) {
        const u32 f = tid % p.F;
        const u32 term = p.terms[(u64)q * TF + tid];
        if (p.imp[f] && term < p.n_terms[f]) {
            const u64 base = p.tf_off[f][term];
            const u32 df = (u32)(p.tf_off[f][term + 1] - base);
            const u32 slot = p.dir_slot[f] ? p.dir_slot[f][term] : 0xFFFFFFFFu;
            u32 lo, hi;
            if (slot != 0xFFFFFFFFu) {
                lo = p.tile_dir[f][(u64)slot * (p.n_tiles + 1) + tile];
                hi = p.tile_dir[f][(u64)slot * (p.n_tiles + 1) + tile + 1u];
            } else {
                lo = sa_lower_bound(p.tfp[f] + base, 0, df, d0 << SA_KEY_SHIFT, SA_KEY_MASK);
                hi = sa_lower_bound(p.tfp[f] + base, lo, df, (d0 + (u64)TILE) << SA_KEY_SHIFT, SA_KEY_MASK);
            }
            first = sa_imp_base(base, term) + lo;
            n = hi - lo;
        }
    }
    s_first[tid] = first; s_n[tid] = n;
    const u32 n_post = sa_block_sum<NW>(n, red);                      // (its barriers publish the table and the zeroed accumulators)
    if (n_post == 0) { if (tid == 0) p.item_cnt[oi] = 0; return; }    // (uniform)

    for (u32 t = 0; t < p.T; t++) {                                   // (uniform control flow throughout)
        bool any = false;
        for (u32 f = 0; f < p.F; f++) {
            const u32 cnt = s_n[t * p.F + f];
            if (cnt == 0) continue;
            if (any) __syncthreads();                                 // another field may hold the same doc in another lane
            any = true;
            const u64 fst = s_first[t * p.F + f];
            const float w = p.w[(u64)q * TF + t * p.F + f];
            const float boost = p.boost[f];
            const int has_boost = p.has_boost[f];
            const u64 SA_AS_GLOBAL* imp = sa_glob(p.imp[f]);
            for (u32 j = tid; j < cnt; j += SA_FB_THREADS) {
                const u64 cell = imp[fst + j];
                const u32 d = ((u32)(cell >> 32) >> 2) - (u32)d0;
                float s = __fmul_rn(__uint_as_float((u32)cell), w);
                if (has_boost) s = __fmul_rn(s, boost);
                if (d < (u32)TILE) {                                  // (always: the slice lies inside the tile)
                    s_sum[d] = __dadd_rn(s_sum[d], (double)s);
                    s_mx[d] = s > s_mx[d] ? s : s_mx[d];
                }
            }
        }
        if (!any) continue;                                           // every doc's clause value is +0.0: total and cnt keep their bits
        __syncthreads();
#pragma unroll
        for (int j = 0; j < E; j++) {
            const u32 e = (u32)j * SA_FB_THREADS + tid;
            const double sum = s_sum[e], mx = (double)s_mx[e];
            const double c = __dadd_rn(mx, __dmul_rn(__dsub_rn(sum, mx), p.tie));
            s_total[e] = __dadd_rn(s_total[e], c);
            s_cnt[e] = (unsigned char)(s_cnt[e] + (c > 0.0 ? 1u : 0u));
            s_sum[e] = 0.0; s_mx[e] = 0.f;
        }
        __syncthreads();
    }
    __syncthreads();

    // mm and fq, found, selection.  From here a thread owns E NEIGHBOURING docs: thread order is doc order.  The E bit patterns live
    // in registers from here on (0: the doc does not rank): the selection's 32 bisection steps re-read them, and neighbouring docs
    // per lane are a 16-way bank conflict in LDS.
    const u32 need = p.need[q];
    u32 npos = 0;
    u64 kreg[E];
#pragma unroll
    for (int j = 0; j < E; j++) {
        const u32 e = tid * (u32)E + (u32)j;
        const double tot = s_total[e];
        bool ok = tot > 0.0 && (u32)s_cnt[e] >= need;
        if (ok && p.fwords) {
            const u64 doc = d0 + e;                                   // (< n_docs: it has a posting)
            ok = (p.fwords[doc >> 5] >> (u32)(doc & 31u)) & 1u;
        }
        kreg[j] = ok ? sa_f64_bits(tot) : 0ull;
        npos += ok ? 1u : 0u;
    }
    const u32 n_found = sa_block_sum<NW>(npos, red);
    if (n_found == 0) { if (tid == 0) p.item_cnt[oi] = 0; return; }   // (uniform)
    if (tid == 0) atomicAdd(&p.found[q], (unsigned long long)n_found);
    auto key = [&](int j) -> u64 { return kreg[j]; };
    u64 thr = 0;                                                      // 0: every positive doc is kept
    if (n_found > p.kk) thr = sa_block_kth_largest<E, NW>(key, p.kk, red64);
    u32 g = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < E; j++) {
        const u64 x = key(j);
        g += x > thr ? 1u : 0u;
        eq += (thr != 0 && x == thr) ? 1u : 0u;
    }
    u32 tot = 0;
    const u32 excl = sa_block_excl_scan<NW>(g | (eq << 16), red, &tot);   // (at most 4096 of either: 16 bits each)
    const u32 n_gt = tot & 0xFFFFu, n_eq = tot >> 16;
    const u32 room = p.kk - n_gt;                                     // (fewer than kk docs lie above the kk-th largest)
    u32 pg = excl & 0xFFFFu, pe = excl >> 16;
    u64* const cb = p.cand_bits + oi * p.kk;
    u32* const cd = p.cand_doc + oi * p.kk;
#pragma unroll
    for (int j = 0; j < E; j++) {
        const u64 x = key(j);
        const u32 doc = (u32)d0 + tid * (u32)E + (u32)j;
        if (x > thr) {
            if (pg < p.kk) { cb[pg] = x; cd[pg] = doc; }
            pg++;
        } else if (thr != 0 && x == thr) {
            if (pe < room) { cb[n_gt + pe] = x; cd[n_gt + pe] = doc; }
            pe++;
        }
    }
    if (tid == 0) p.item_cnt[oi] = n_gt + (n_eq < room ? n_eq : room);
}

// ---- merge: the k best of a query's candidates --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
sa_k_fields_merge(const u64* __restrict__ cand_bits, const u32* __restrict__ cand_doc, const u32* __restrict__ item_cnt, u32 n_tiles,
                  u32 kk, u32 k, u32 q0, u64* __restrict__ out_scores, u64* __restrict__ out_rows) {
    __shared__ u64 sv[SA_FB_MERGE_LIST];
    __shared__ u32 sd[SA_FB_MERGE_LIST];
    __shared__ u32 s_np, s_td;
    __shared__ u64 s_tb;
    const u32 tid = threadIdx.x, nthr = blockDim.x;
    const u32 ql = blockIdx.x;
    u32 KB = 32;                                                      // the sorted best live in [0, KB), pending candidates behind them
    while (KB < k) KB <<= 1;
    const u32 P = SA_FB_MERGE_LIST - KB;                              // (>= 3072: at least three rounds of candidates)
    for (u32 i = tid; i < SA_FB_MERGE_LIST; i += nthr) { sv[i] = 0ull; sd[i] = 0xFFFFFFFFu; }
    if (tid == 0) { s_np = 0; s_tb = 0ull; s_td = 0; }
    __syncthreads();
    const u32 n_slots = n_tiles * kk;
    const u64* const cb = cand_bits + (u64)ql * n_slots;
    const u32* const cd = cand_doc + (u64)ql * n_slots;
    const u32* const ic = item_cnt + (u64)ql * n_tiles;
    for (u32 base = 0; base < n_slots; base += nthr) {                // (uniform trip count)
        const u32 s = base + tid;
        if (s < n_slots) {
            const u32 tile = s / kk, j = s - tile * kk;
            if (j < ic[tile]) {
                const u64 x = cb[s];
                const u32 d = cd[s];
                const u64 tb = s_tb;                                  // the k-th best so far (0: fewer than k yet)
                if (x > tb || (x == tb && d < s_td)) {
                    const u32 pos = atomicAdd(&s_np, 1u);             // (room for a whole round is kept free below)
                    sv[KB + pos] = x; sd[KB + pos] = d;
                }
            }
        }
        __syncthreads();
        const u32 np = s_np;
        __syncthreads();                                              // (everyone has read the count before anyone appends again)
        const bool last = base + nthr >= n_slots;
        if (np == 0 || !(last || np + nthr > P)) continue;            // (uniform)
        u32 n2 = 2;
        while (n2 < KB + np) n2 <<= 1;
        for (u32 size = 2; size <= n2; size <<= 1) {
            for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                for (u32 t = tid; t < (n2 >> 1); t += nthr) {
                    const u32 lo = 2 * t - (t & (stride - 1));
                    const u32 hi = lo + stride;
                    const bool desc = ((lo & size) == 0);
                    const u64 xv = sv[lo], yv = sv[hi];
                    const u32 xi = sd[lo], yi = sd[hi];
                    const bool x_first = xv > yv || (xv == yv && xi < yi);    // bits descending, then doc ascending
                    if (desc ? !x_first : x_first) { sv[lo] = yv; sv[hi] = xv; sd[lo] = yi; sd[hi] = xi; }
                }
            }
        }
        __syncthreads();
        for (u32 i = KB + tid; i < n2; i += nthr) { sv[i] = 0ull; sd[i] = 0xFFFFFFFFu; }
        if (tid == 0) {
            s_np = 0;
            if (sv[k - 1] != 0ull) { s_tb = sv[k - 1]; s_td = sd[k - 1]; }
        }
        __syncthreads();
    }
    const u64 ob = (u64)(q0 + ql) * k;
    for (u32 i = tid; i < k; i += nthr) {
        const u64 x = sv[i];
        out_scores[ob + i] = x;
        out_rows[ob + i] = x != 0ull ? (u64)sd[i] : SA_NO_DOC;
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct sa_fields_batch {
    sa_options_t opts;
    int device = 0;
    u32 F = 0, tile = 0, n_tiles = 0;
    u64 n_docs = 0;
    sa_index* ix[SA_FB_MAXF] = {};
    std::shared_ptr<sa_impacts> imp[SA_FB_MAXF];
    float boost[SA_FB_MAXF] = {};
    int has_boost[SA_FB_MAXF] = {};
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_up = nullptr;
    std::shared_ptr<sa_filter_data> filter;
    // the loaded query set
    u32 B = 0, T = 0, k = 0, kk = 0, q_slice = 0;
    double tie = 0.0;
    bool loaded = false, ran = false, up_pending = false, prof_pending = false;
    // one upload block (terms | weights | need) with its page-locked image; results (scores | rows | found) with theirs; candidates
    char* d_up = nullptr; char* h_up = nullptr; size_t up_cap = 0;
    char* d_out = nullptr; char* h_out = nullptr; size_t out_cap = 0;
    char* d_cand = nullptr; size_t cand_cap = 0;
    u64 alg_bytes = 0;
    u32 slices = 0;
    double last_ms = 0.0;
    std::mutex mu;                               // one call at a time per batch
};

static size_t sa_fb_up_bytes(u32 B, u32 T, u32 F) { return (size_t)B * T * F * 8 + (size_t)B * 4; }
static size_t sa_fb_out_bytes(u32 B, u32 k) { return (size_t)B * k * 16 + (size_t)B * 8; }
// candidate bytes of one query in flight: (bits, doc) x kk per tile + the item counts, the u64 part first
static size_t sa_fb_cand_bytes(u32 n_tiles, u32 kk) { return (size_t)n_tiles * kk * 12 + (size_t)n_tiles * 4; }

static void sa_fields_free(sa_fields_batch* fb) {
    hipSetDevice(fb->device);
    if (fb->st) hipStreamSynchronize(fb->st);
    if (fb->d_up) hipFree(fb->d_up);
    if (fb->h_up) hipHostFree(fb->h_up);
    if (fb->d_out) hipFree(fb->d_out);
    if (fb->h_out) hipHostFree(fb->h_out);
    if (fb->d_cand) hipFree(fb->d_cand);
    if (fb->ev0) hipEventDestroy(fb->ev0);
    if (fb->ev1) hipEventDestroy(fb->ev1);
    if (fb->ev_up) hipEventDestroy(fb->ev_up);
    if (fb->st) hipStreamDestroy(fb->st);
    delete fb;
}

extern "C" int sa_fields_batch_create(sa_index_t* const* fields, int n_fields, const float* k1, const float* b, const float* boost,
                                      const int32_t* has_boost, sa_fields_batch_t** out) {
    SA_ARG(fields && k1 && b && boost && has_boost && out, "null argument");
    SA_ARG(n_fields >= 1 && n_fields <= SA_FB_MAXF, "a fields batch spans 1 .. 8 indexes");
    for (int f = 0; f < n_fields; f++) {
        SA_ARG(fields[f], "null index");
        SA_ARG(fields[f]->device == fields[0]->device, "the fields' indexes live on different devices");
        SA_ARG(fields[f]->n_docs == fields[0]->n_docs, "the fields' indexes hold different numbers of documents");
        SA_ARG(fields[f]->doc_base == 0 && !fields[f]->comm, "a fields batch takes whole indexes (doc_base 0, no communicator)");
    }
    SA_ARG(fields[0]->n_docs > 0 && fields[0]->n_docs < (1ull << 32), "n_docs must be in 1 .. 2^32 - 1");
    sa_fields_batch* fb = new (std::nothrow) sa_fields_batch();
    if (!fb) { sa_set_error("out of host memory"); return SA_ERR_NOMEM; }
    fb->opts = sa_options_for_new_handle(&fields[0]->opts);
    fb->device = fields[0]->device;
    fb->F = (u32)n_fields;
    fb->n_docs = fields[0]->n_docs;
    const u32 t0 = fields[0]->tile_docs;
    fb->tile = (t0 == 1024 || t0 == 2048 || t0 == 4096) ? t0 : SA_DEFAULT_TILE_DOCS;
    fb->n_tiles = sa_div_up(fb->n_docs, fb->tile);
    int rc = SA_OK;
    for (int f = 0; f < n_fields && rc == SA_OK; f++) {
        sa_index* ix = fields[f];
        fb->ix[f] = ix; fb->boost[f] = boost[f]; fb->has_boost[f] = has_boost[f] ? 1 : 0;
        std::lock_guard<std::mutex> g(ix->mu);                        // (one index lock at a time)
        if (hipSetDevice(ix->device) != hipSuccess) { sa_set_error("hipSetDevice failed"); rc = SA_ERR_HIP; break; }
        fb->imp[f] = sa_impacts_get(ix, k1[f], b[f], fb->opts);
        if (!fb->imp[f] || !fb->imp[f]->d_imp) {
            fb->imp[f] = nullptr;
            // sa_index_bm25_dense emits zeros for such a field; anything else the caller answers query by query
            if (!(ix->n_postings == 0 || ix->n_terms == 0 || ix->avg_doc_len == 0.f)) {
                sa_set_error("sa_fields_batch_create: field %d has no impact stream (option impact = 0, or device memory is short)", f);
                rc = SA_ERR_UNSUPPORTED;
            }
        } else if (hipStreamSynchronize(ix->stream) != hipSuccess) {  // (a new stream is built on the index's stream; this batch has its own)
            sa_set_error("sa_fields_batch_create: hipStreamSynchronize failed");
            rc = SA_ERR_HIP;
        }
    }
    if (rc == SA_OK && (hipStreamCreateWithFlags(&fb->st, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&fb->ev0) != hipSuccess ||
                        hipEventCreate(&fb->ev1) != hipSuccess || hipEventCreateWithFlags(&fb->ev_up, hipEventDisableTiming) != hipSuccess)) {
        sa_set_error("sa_fields_batch_create: stream / event creation failed");
        rc = SA_ERR_HIP;
    }
    if (rc != SA_OK) { sa_fields_free(fb); return rc; }
    *out = fb;
    return SA_OK;
}

// make room for a (B, T, k) query set: nothing happens when the buffers are large enough
static int sa_fields_reserve(sa_fields_batch* fb, u32 B, u32 T, u32 k) {
    const u32 kk = k < fb->tile ? k : fb->tile;
    const size_t up = sa_fb_up_bytes(B, T, fb->F), ob = sa_fb_out_bytes(B, k), per_q = sa_fb_cand_bytes(fb->n_tiles, kk);
    const long long mb = std::max<long long>(1, sa_opt(fb->opts.fields_cand_mb, SA_FB_DEFAULT_CAND_MB));
    u64 qs = ((u64)mb << 20) / per_q;
    qs = qs < 1 ? 1 : (qs > B ? B : qs);
    const size_t cb = (size_t)qs * per_q;
    if (up > fb->up_cap || ob > fb->out_cap || cb > fb->cand_cap) SA_HIP(hipStreamSynchronize(fb->st));
    if (up > fb->up_cap) {
        if (fb->d_up) { hipFree(fb->d_up); fb->d_up = nullptr; }
        if (fb->h_up) { hipHostFree(fb->h_up); fb->h_up = nullptr; }
        fb->up_cap = 0;
        SA_HIP(hipMalloc((void**)&fb->d_up, up));
        SA_HIP(hipHostMalloc((void**)&fb->h_up, up));
        fb->up_cap = up;
    }
    if (ob > fb->out_cap) {
        if (fb->d_out) { hipFree(fb->d_out); fb->d_out = nullptr; }
        if (fb->h_out) { hipHostFree(fb->h_out); fb->h_out = nullptr; }
        fb->out_cap = 0;
        SA_HIP(hipMalloc((void**)&fb->d_out, ob));
        SA_HIP(hipHostMalloc((void**)&fb->h_out, ob));
        fb->out_cap = ob;
    }
    if (cb > fb->cand_cap) {
        if (fb->d_cand) { hipFree(fb->d_cand); fb->d_cand = nullptr; }
        fb->cand_cap = 0;
        SA_HIP(hipMalloc((void**)&fb->d_cand, cb));
        fb->cand_cap = cb;
    }
    fb->kk = kk;
    fb->q_slice = (u32)qs;
    return SA_OK;
}

extern "C" int sa_fields_batch_set_queries(sa_fields_batch_t* fb, const uint32_t* terms, const float* weights, const uint32_t* need,
                                           int n_queries, int n_clauses, int k, double tie) {
    SA_ARG(fb && terms && weights && need, "null argument");
    SA_ARG(n_queries >= 1, "n_queries < 1");
    SA_ARG(n_clauses >= 1 && n_clauses <= SA_MAX_QTERMS, "a query has 1 .. 32 clauses");
    SA_ARG(k >= 1 && k <= SA_KMAX, "k must be in 1 .. SA_KMAX");
    std::lock_guard<std::mutex> g(fb->mu);
    SA_HIP(hipSetDevice(fb->device));
    const u32 B = (u32)n_queries, T = (u32)n_clauses, F = fb->F;
    fb->loaded = false;
    SA_TRY(sa_fields_reserve(fb, B, T, (u32)k));
    if (fb->up_pending) { SA_HIP(hipEventSynchronize(fb->ev_up)); fb->up_pending = false; }   // (the image is free again)
    const size_t n = (size_t)B * T * F;
    memcpy(fb->h_up, terms, n * 4);
    memcpy(fb->h_up + n * 4, weights, n * 4);
    memcpy(fb->h_up + n * 8, need, (size_t)B * 4);
    SA_HIP(hipMemcpyAsync(fb->d_up, fb->h_up, sa_fb_up_bytes(B, T, F), hipMemcpyHostToDevice, fb->st));
    SA_HIP(hipEventRecord(fb->ev_up, fb->st));
    fb->up_pending = true;
    // algorithmic bytes of a run: 8 x the postings of every (query, clause, field) term (the index's host offsets never change)
    u64 postings = 0;
    for (size_t i = 0; i < n; i++) {
        const u32 f = (u32)(i % F), term = terms[i];
        const sa_index* ix = fb->ix[f];
        if (fb->imp[f] && term < ix->n_terms) postings += ix->h_tf_off[term + 1] - ix->h_tf_off[term];
    }
    fb->alg_bytes = 8ull * postings;
    fb->B = B; fb->T = T; fb->k = (u32)k; fb->tie = tie;
    fb->loaded = true; fb->ran = false;
    return SA_OK;
}

extern "C" int sa_fields_batch_set_filter(sa_fields_batch_t* fb, sa_filter_t* f) {
    SA_ARG(fb, "null batch");
    SA_ARG(!f || f->d, "null filter");
    SA_ARG(!f || f->d->device == fb->device, "the filter lives on another device than the batch's indexes");
    SA_ARG(!f || f->d->n_docs == fb->n_docs, "the filter covers another number of documents than the batch's indexes hold");
    std::lock_guard<std::mutex> g(fb->mu);
    SA_HIP(hipSetDevice(fb->device));
    if (fb->filter) SA_HIP(hipStreamSynchronize(fb->st));             // (runs in flight read the bitmap this call may release)
    fb->filter = f ? f->d : nullptr;
    return SA_OK;
}

extern "C" int sa_fields_batch_run(sa_fields_batch_t* fb, int sync) {
    SA_ARG(fb, "null batch");
    std::lock_guard<std::mutex> g(fb->mu);
    if (!fb->loaded) { sa_set_error("sa_fields_batch_run: no query set (sa_fields_batch_set_queries)"); return SA_ERR_STATE; }
    SA_HIP(hipSetDevice(fb->device));
    hipStream_t st = fb->st;
    const u32 B = fb->B, k = fb->k, kk = fb->kk, F = fb->F, T = fb->T;
    FieldsParams p;
    memset(&p, 0, sizeof(p));
    for (u32 f = 0; f < F; f++) {
        const sa_index* ix = fb->ix[f];
        p.tfp[f] = ix->d_tfp; p.tf_off[f] = ix->d_tf_off;
        const bool dir = ix->tile_docs == fb->tile && ix->n_tiles == fb->n_tiles && ix->d_dir_slot && ix->d_tile_dir;
        p.dir_slot[f] = dir ? ix->d_dir_slot : nullptr;
        p.tile_dir[f] = dir ? ix->d_tile_dir : nullptr;
        p.imp[f] = fb->imp[f] ? fb->imp[f]->d_imp : nullptr;
        p.n_terms[f] = ix->n_terms;
        p.boost[f] = fb->boost[f]; p.has_boost[f] = fb->has_boost[f];
    }
    p.F = F; p.T = T; p.n_tiles = fb->n_tiles; p.k = k; p.kk = kk; p.n_docs = fb->n_docs; p.tie = fb->tie;
    const size_t n = (size_t)B * T * F;
    p.terms = (const u32*)fb->d_up;
    p.w = (const float*)(fb->d_up + n * 4);
    p.need = (const u32*)(fb->d_up + n * 8);
    if (fb->filter) {
        p.fwords = (const u32*)fb->filter->d_words;
        p.fblk = fb->filter->d_blk;
        p.n_fblocks = fb->filter->n_blocks;
    }
    const u32 qs = fb->q_slice;
    p.cand_bits = (u64*)fb->d_cand;
    p.cand_doc = (u32*)(fb->d_cand + (size_t)qs * fb->n_tiles * kk * 8);
    p.item_cnt = p.cand_doc + (size_t)qs * fb->n_tiles * kk;
    u64* const d_scores = (u64*)fb->d_out;
    u64* const d_rows = d_scores + (size_t)B * k;
    p.found = (unsigned long long*)(d_rows + (size_t)B * k);
    SA_HIP(hipMemsetAsync(p.found, 0, (size_t)B * 8, st));
    SA_HIP(hipEventRecord(fb->ev0, st));
    const u32 n_slots = fb->n_tiles * kk;
    const u32 merge_threads = n_slots > 8192u ? 1024u : 256u;
    u32 slices = 0;
    for (u32 q0 = 0; q0 < B; q0 += qs, slices++) {
        p.q0 = q0; p.nq = B - q0 < qs ? B - q0 : qs;
        const dim3 grid(p.nq * fb->n_tiles);
        if (fb->tile == 1024) hipLaunchKernelGGL((sa_k_fields_score<1024>), grid, dim3(SA_FB_THREADS), 0, st, p);
        else if (fb->tile == 2048) hipLaunchKernelGGL((sa_k_fields_score<2048>), grid, dim3(SA_FB_THREADS), 0, st, p);
        else hipLaunchKernelGGL((sa_k_fields_score<4096>), grid, dim3(SA_FB_THREADS), 0, st, p);
        hipLaunchKernelGGL(sa_k_fields_merge, dim3(p.nq), dim3(merge_threads), 0, st, (const u64*)p.cand_bits, (const u32*)p.cand_doc,
                           (const u32*)p.item_cnt, fb->n_tiles, kk, k, q0, d_scores, d_rows);
    }
    SA_HIP(hipGetLastError());
    SA_HIP(hipEventRecord(fb->ev1, st));
    fb->slices = slices;
    fb->prof_pending = true;
    fb->ran = true;
    if (sa_opt(fb->opts.trace, 0))
        fprintf(stderr, "sa_fields_batch_run: %u queries x %u clauses x %u fields, %u tiles of %u docs, k %u, %u slice(s) of %u\n", B, T, F,
                fb->n_tiles, fb->tile, k, slices, qs);
    if (sync) SA_HIP(hipStreamSynchronize(st));
    return SA_OK;
}

extern "C" int sa_fields_batch_fetch(sa_fields_batch_t* fb, double* scores_out, uint64_t* rows_out, uint64_t* found_out) {
    SA_ARG(fb && scores_out && rows_out, "null argument");
    std::lock_guard<std::mutex> g(fb->mu);
    if (!fb->ran) { sa_set_error("sa_fields_batch_fetch: the loaded query set has not been run"); return SA_ERR_STATE; }
    SA_HIP(hipSetDevice(fb->device));
    const size_t nk = (size_t)fb->B * fb->k;
    SA_HIP(hipMemcpyAsync(fb->h_out, fb->d_out, sa_fb_out_bytes(fb->B, fb->k), hipMemcpyDeviceToHost, fb->st));
    SA_HIP(hipStreamSynchronize(fb->st));
    memcpy(scores_out, fb->h_out, nk * 8);
    memcpy(rows_out, fb->h_out + nk * 8, nk * 8);
    if (found_out) memcpy(found_out, fb->h_out + nk * 16, (size_t)fb->B * 8);
    return SA_OK;
}

extern "C" int sa_fields_batch_profile(sa_fields_batch_t* fb, double* kernel_ms_out, uint64_t* alg_bytes_out, uint32_t* slices_out) {
    SA_ARG(fb, "null batch");
    std::lock_guard<std::mutex> g(fb->mu);
    if (fb->prof_pending) {
        SA_HIP(hipSetDevice(fb->device));
        SA_HIP(hipEventSynchronize(fb->ev1));
        float ms = 0.f;
        SA_HIP(hipEventElapsedTime(&ms, fb->ev0, fb->ev1));
        fb->last_ms = (double)ms;
        fb->prof_pending = false;
    }
    if (kernel_ms_out) *kernel_ms_out = fb->last_ms;
    if (alg_bytes_out) *alg_bytes_out = fb->alg_bytes;
    if (slices_out) *slices_out = fb->slices;
    return SA_OK;
}

extern "C" int sa_fields_batch_destroy(sa_fields_batch_t* fb) {
    if (!fb) return SA_OK;
    sa_fields_free(fb);
    return SA_OK;
}
