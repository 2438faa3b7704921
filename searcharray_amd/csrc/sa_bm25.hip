// sa_bm25.hip -- term-at-a-time BM25 over the HBM-resident TF postings, with per-tile and
// per-query top-k.
//
// Replaces the reference's per-term dense pipeline
//     as_dense (scatter, roaringish_ops.pyx:84-98)  ->  _bm25_score (bm25.pyx:11-25, O(N) per term)
//     ->  np.sum(axis=0) (test/test_msmarco.py:353-354)  ->  np.argpartition (utils/sort.py:24)
// with one sparse pass: a workgroup owns (query, doc tile); the tile's fp32 score accumulators
// live in LDS; each query term's slice of the posting stream -- the fat TF postings (doc|doc_len|tf
// in one u64) or, for top-k batches, the impact stream derived from them (doc*4 | fp32 factor) -- is
// read once with coalesced 16-byte loads, scored, and added into LDS in QUERY-TERM ORDER (a barrier
// separates terms) so the fp32 sum is bit-identical to the reference's ((s0+s1)+s2)+s3.
// Per-posting arithmetic is the reference's, op for op, each rounded to fp32 (no FMA contraction,
// IEEE division):  tf / (tf + k1 * ((1 - b) + b * (dl / avgdl))) * idf.
//
// Roofline: HBM-bound integer/bitwise + scalar fp32 work (no MFMA).  Algorithmic bytes per query
// = sum_t 8 * df_t (+ 4 * n_docs the reference-style doc_lens pass would read; this layout folds
// doc_len into the posting so the real traffic is lower).
#include "sa_index.hpp"
#include "sa_topk.hpp"
#include "sa_batch.hpp"
#include "sa_bm25_params.hpp"
#include "sa_facet.hpp"
#include "../../include/searcharray_hip.h"

#include <algorithm>
#include <type_traits>
#include <new>
#include <stdlib.h>
#include <math.h>


// ---- impact stream ---------------------------------------------------------------------------------
// The exhaustive tile kernel is bound by instruction issue per posting, not by posting bytes.
// Everything of a posting's score except the final `* idf` depends only on (tf, doc_len) and the batch
// constants k1, b, avgdl, so it is evaluated ONCE per (k1, b) for the whole shard -- with the reference's
// operation order (bm25.pyx:19-23), so the bits are the ones the per-posting arithmetic would give -- and
// kept beside the TF postings in the layout the tile kernel wants (sa_impacts in sa_index.hpp): per
// posting the kernel is left with a subtract, a compare, a multiply and the LDS read-modify-write.
sa_impacts::~sa_impacts() {
    if (d_imp || d_dense) hipSetDevice(device);
    if (d_imp) hipFree(d_imp);
    if (d_dense) hipFree(d_dense);
    if (d_topf) hipFree(d_topf);
    if (d_maxf) hipFree(d_maxf);
    if (d_probe) hipFree(d_probe);
    if (d_pbits) hipFree(d_pbits);
}

// dense factor row of one term (sa_impacts::d_dense): row[doc] = factor bits of the term's posting of doc; the row is zeroed before
__global__ void __launch_bounds__(256)
sa_k_make_dense_row(const u64* __restrict__ imp, u64 first, u64 df, float* __restrict__ row) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < df; i += (u64)gridDim.x * blockDim.x) {
        const u64 c = imp[first + i];
        row[(u32)(c >> 32) >> 2] = __uint_as_float((u32)c);
    }
}

// (sa_imp_base / sa_imp_sentinel: sa_bm25_params.hpp)

// Rank table of a term's factors (sa_impacts::d_topf): one workgroup per term builds a histogram of its postings' factor
// bits -- 512 bins per octave over [1/16, 1): (bits >> 14) - (123 << 9), clamped -- and reads off, from the top, the bin
// that holds the r-th largest factor for each tabulated rank r; the bin's LOWER edge is what is stored.
#define SA_TOPF_BINS 2048
#define SA_TOPF_LO (123u << 9)
#define SA_TOPF_SLICE 65536ull          // postings per workgroup of a LONG list's histogram (lists of 4 slices and more; option topf_slice: test hook)
struct TopfRanks { u32 r[SA_TOPF_NR]; };
__global__ void __launch_bounds__(256)
sa_k_topf_hist_long(const u64* __restrict__ imp, const u64* __restrict__ tf_off, const u32* __restrict__ slice_term,
                    const u32* __restrict__ slice_first, const u32* __restrict__ long_slot, u32* __restrict__ ghist, u32* __restrict__ gmax, const u64 slice) {
    // one workgroup per SLICE (SA_TOPF_SLICE postings) of a LONG list: its histogram in LDS, added to the term's row of `ghist`
    __shared__ u32 s_h[SA_TOPF_BINS];
    const u32 tid = threadIdx.x, t = slice_term[blockIdx.x];
    const u64 base = tf_off[t], df = tf_off[t + 1] - base;
    const u64 i0 = (u64)slice_first[blockIdx.x] * slice, i1 = i0 + slice < df ? i0 + slice : df;
    for (u32 i = tid; i < (u32)SA_TOPF_BINS; i += 256) s_h[i] = 0;
    __syncthreads();
    const u64* const cells = imp + sa_imp_base(base, t);
    u32 mx = 0u;
    for (u64 i = i0 + tid; i < i1; i += 256) {
        const u32 fb = (u32)cells[i];
        mx = fb > mx ? fb : mx;
        const u32 e = fb >> 14;
        const u32 b = e <= SA_TOPF_LO ? 0u : (e - SA_TOPF_LO > (u32)(SA_TOPF_BINS - 1) ? (u32)(SA_TOPF_BINS - 1) : e - SA_TOPF_LO);
        atomicAdd(&s_h[b], 1u);
    }
    __syncthreads();
    u32* const row = ghist + (u64)long_slot[t] * SA_TOPF_BINS;
    for (u32 i = tid; i < (u32)SA_TOPF_BINS; i += 256) if (s_h[i]) atomicAdd(&row[i], s_h[i]);
    if (mx) atomicMax(&gmax[long_slot[t]], mx);
}

// (long_slot: [n_terms] row of a LONG term in ghist / gmax -- its histogram is there already, sa_k_topf_hist_long -- else all ones; or null)
__global__ void __launch_bounds__(256)
sa_k_make_topf(const u64* __restrict__ imp, const u64* __restrict__ tf_off, u32 n_terms, const TopfRanks ranks, float* __restrict__ topf,
               float* __restrict__ maxf, const u32* __restrict__ long_slot, const u32* __restrict__ ghist, const u32* __restrict__ gmax) {
    __shared__ u32 s_h[SA_TOPF_BINS];
    __shared__ u32 s_part[256];
    __shared__ u32 s_max;
    const u32 tid = threadIdx.x;
    for (u32 t = blockIdx.x; t < n_terms; t += gridDim.x) {
        const u64 base = tf_off[t], df = tf_off[t + 1] - base;
        float* const row = topf + (u64)t * SA_TOPF_NR;
        if (df == 0) {                                           // (uniform)
            if (tid < (u32)SA_TOPF_NR) row[tid] = 0.f;
            if (tid == 0 && maxf) maxf[t] = 0.f;
            continue;
        }
        const u32 ls = long_slot ? long_slot[t] : 0xFFFFFFFFu;     // (uniform)
        for (u32 i = tid; i < (u32)SA_TOPF_BINS; i += 256) s_h[i] = ls != 0xFFFFFFFFu ? ghist[(u64)ls * SA_TOPF_BINS + i] : 0u;
        if (tid == 0) s_max = ls != 0xFFFFFFFFu ? gmax[ls] : 0u;
        __syncthreads();
        const u64* const cells = imp + sa_imp_base(base, t);
        u32 mx = 0u;                                             // (factors are non-negative: their bit patterns order like the values)
        for (u64 i = tid; i < (ls != 0xFFFFFFFFu ? 0ull : df); i += 256) {
            const u32 fb = (u32)cells[i];
            mx = fb > mx ? fb : mx;
            const u32 e = fb >> 14;
            const u32 b = e <= SA_TOPF_LO ? 0u : (e - SA_TOPF_LO > (u32)(SA_TOPF_BINS - 1) ? (u32)(SA_TOPF_BINS - 1) : e - SA_TOPF_LO);
            atomicAdd(&s_h[b], 1u);
        }
        if (mx) atomicMax(&s_max, mx);
        __syncthreads();
        if (tid == 0 && maxf) maxf[t] = __uint_as_float(s_max);
        // thread i owns bins [8 i, 8 i + 8); above[i] = postings in the bins above its eight
        u32 mine = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) mine += s_h[tid * 8u + (u32)j];
        s_part[tid] = mine;
        __syncthreads();
        u32 above = 0;
        for (u32 j = tid + 1; j < 256; j++) above += s_part[j];
        // bin b holds the r-th largest iff  count(bins > b) < r <= count(bins >= b)
        u32 cum = above;
        for (int j = 7; j >= 0; j--) {
            const u32 b = tid * 8u + (u32)j;
            const u32 c = s_h[b];
            for (int x = 0; x < SA_TOPF_NR; x++)
                if (c && cum < ranks.r[x] && ranks.r[x] <= cum + c)
                    row[x] = b == 0u ? 0.f : __uint_as_float((b + SA_TOPF_LO) << 14);
            cum += c;
        }
        // ranks beyond the term's postings: no bound
        if (tid < (u32)SA_TOPF_NR && ranks.r[tid] > df) row[tid] = 0.f;
        __syncthreads();
    }
}


__global__ void __launch_bounds__(256)
sa_k_make_impacts(const u64* __restrict__ tfp, const u64* __restrict__ tf_off, const float* __restrict__ doc_lens,
                  u32 n_terms, u64 n_postings, int dl_packed, float k1, float b, float avgdl, u64* __restrict__ imp) {
    constexpr u32 CHUNK = 2048;
    __shared__ u32 s_t[2];
    const float one_minus_b = 1.0f - b;
    const u64 n_chunks = (n_postings + CHUNK - 1) / CHUNK;
    for (u64 c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const u64 first = c * CHUNK;
        const u64 last = first + CHUNK <= n_postings ? first + CHUNK - 1 : n_postings - 1;
        // terms of the chunk's first and last posting: largest t with tf_off[t] <= i
        if (threadIdx.x < 2) {
            const u64 i = threadIdx.x == 0 ? first : last;
            u32 lo = 0, hi = n_terms;                  // answer in [lo, hi)
            while (hi - lo > 1) {
                const u32 mid = lo + (hi - lo) / 2;
                if (tf_off[mid] <= i) lo = mid; else hi = mid;
            }
            s_t[threadIdx.x] = lo;
        }
        __syncthreads();
        const u32 t_first = s_t[0], t_last = s_t[1];
        for (u64 i = first + threadIdx.x; i <= last; i += blockDim.x) {
            u32 lo = t_first, hi = t_last + 1;
            while (hi - lo > 1) {
                const u32 mid = lo + (hi - lo) / 2;
                if (tf_off[mid] <= i) lo = mid; else hi = mid;
            }
            const u64 tbase = tf_off[lo];
            const u64 x = tfp[i];
            const u32 doc = (u32)(x >> SA_KEY_SHIFT);
            const float tf = (float)(u32)(x & SA_LSB_MASK);
            const float dl = dl_packed ? (float)(u32)((x >> SA_LSB_BITS) & SA_LSB_MASK) : doc_lens[doc];
            const float norm = __fmul_rn(k1, __fadd_rn(one_minus_b, __fmul_rn(b, __fdiv_rn(dl, avgdl))));
            const float sat = __fdiv_rn(tf, __fadd_rn(tf, norm));
            imp[sa_imp_base(tbase, lo) + (i - tbase)] = ((u64)(doc << 2) << 32) | (u64)__float_as_uint(sat);   // doc * 4: the accumulator's byte offset
        }
        __syncthreads();
    }
}

// The impact stream of (k1, b) for this index: the cached one, or a new one (the cache keeps the most
// recent; batches built earlier keep theirs alive).  Null when switched off (option impact = 0), for an empty
// shard, or when HBM is short -- the tile kernel then scores the TF postings.  Call with the index lock held.
std::shared_ptr<sa_impacts> sa_impacts_get(sa_index* ix, float k1, float b, const sa_options_t& o) {
    if (sa_opt(o.impact, 1) == 0) return nullptr;
    if (ix->n_postings == 0 || ix->n_terms == 0 || ix->avg_doc_len == 0.f) return nullptr;
    // (bit patterns: a NaN parameter must still find its own stream)
    auto same = [](float x, float y) { return memcmp(&x, &y, sizeof(float)) == 0; };
    if (ix->impacts && same(ix->impacts->k1, k1) && same(ix->impacts->b, b) && same(ix->impacts->avgdl, ix->avg_doc_len))
        return ix->impacts;
    std::shared_ptr<sa_impacts> im(new (std::nothrow) sa_impacts());
    if (!im) return nullptr;
    im->device = ix->device; im->k1 = k1; im->b = b; im->avgdl = ix->avg_doc_len;
    im->n = sa_imp_base(ix->n_postings, ix->n_terms) + 4;
    if (hipMalloc(&im->d_imp, im->n * sizeof(u64)) != hipSuccess) {
        (void)hipGetLastError();
        im->d_imp = nullptr;
        return nullptr;
    }
    hipStream_t st = ix->stream;
    if (hipMemsetAsync(im->d_imp, 0xFF, im->n * sizeof(u64), st) != hipSuccess) return nullptr;
    const u64 n_chunks = (ix->n_postings + 2047) / 2048;
    const u32 grid = n_chunks < 16384 ? (u32)n_chunks : 16384u;
    hipLaunchKernelGGL(sa_k_make_impacts, dim3(grid), dim3(256), 0, st, ix->d_tfp, ix->d_tf_off, ix->d_doc_lens,
                       ix->n_terms, ix->n_postings, ix->dl_packed ? 1 : 0, k1, b, ix->avg_doc_len, im->d_imp);
    if (hipGetLastError() != hipSuccess) return nullptr;
    // the stream's last pair: a sentinel with the factor 0.0 (doc field all ones like every sentinel) -- what the grouped
    // kernel's empty half entries point at: their lanes add 0 to their spare slots instead of a NaN
    static const u64 tail[2] = {0xFFFFFFFF00000000ull, 0xFFFFFFFF00000000ull};
    if (hipMemcpyAsync(im->d_imp + im->n - 2, tail, sizeof(tail), hipMemcpyHostToDevice, st) != hipSuccess) return nullptr;
    // dense factor rows of the terms with df >= n_docs / dense_div (index option; default 4; 0: none), at most 16, most frequent first
    im->dense_slot.assign(ix->n_terms, 0xFFFFFFFFu);
    {
        const int div = (int)sa_opt(ix->opts.dense_div, 4);
        std::vector<std::pair<u64, u32>> cand;
        if (div > 0 && ix->n_tiles > 0)
            for (u32 t = 0; t < ix->n_terms; t++) {
                const u64 df = ix->h_tf_off[t + 1] - ix->h_tf_off[t];
                if (df * (u64)div >= ix->n_docs && df > 0) cand.push_back({df, t});
            }
        std::sort(cand.begin(), cand.end(), [](const std::pair<u64, u32>& a, const std::pair<u64, u32>& c) { return a.first > c.first || (a.first == c.first && a.second < c.second); });
        if (cand.size() > 16) cand.resize(16);
        if (!cand.empty()) {
            im->dense_stride = (u64)ix->n_tiles * ix->tile_docs;
            const size_t bytes = cand.size() * im->dense_stride * sizeof(float);
            if (hipMalloc(&im->d_dense, bytes) == hipSuccess && hipMemsetAsync(im->d_dense, 0, bytes, st) == hipSuccess) {
                for (size_t r = 0; r < cand.size(); r++) {
                    const u32 t = cand[r].second;
                    const u64 df = cand[r].first;
                    const u32 grid = df / 256 + 1 < 8192 ? (u32)(df / 256 + 1) : 8192u;
                    hipLaunchKernelGGL(sa_k_make_dense_row, dim3(grid), dim3(256), 0, st, (const u64*)im->d_imp,
                                       sa_imp_base(ix->h_tf_off[t], t), df, im->d_dense + r * im->dense_stride);
                    im->dense_slot[t] = (u32)r;
                }
                im->n_dense = (u32)cand.size();
            } else {
                (void)hipGetLastError();
                if (im->d_dense) { hipFree(im->d_dense); im->d_dense = nullptr; }   // (HBM short: the postings serve)
            }
        }
    }
    ix->impacts = im;
    return im;
}

// Rank table of every term's factors (sa_impacts::d_topf: 88 bytes per term), built when the FIRST batch that can use starting
// bounds asks for it -- not with the stream: a batch with term_seed = 0, with k > 1024 or on the pruning route never reads it.
// Tried once per stream; when HBM is short the batches start from 0 as before round 4.  Call with the index lock held.
void sa_impacts_ensure_topf(sa_index* ix, sa_impacts* im) {
    if (!im || im->d_topf || im->topf_tried) return;
    im->topf_tried = true;
    const size_t bytes = (size_t)ix->n_terms * SA_TOPF_NR * sizeof(float);
    if (hipMalloc(&im->d_topf, bytes) != hipSuccess) { (void)hipGetLastError(); im->d_topf = nullptr; return; }
    TopfRanks rk;
    for (int i = 0; i < SA_TOPF_NR; i++) rk.r[i] = sa_topf_ranks[i];
    if (hipMalloc(&im->d_maxf, (size_t)ix->n_terms * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); im->d_maxf = nullptr; }
    // Long lists (4 slices of 64 K postings and more) are histogrammed slice by slice first: with one workgroup per TERM the ten longest
    // lists of a 10 M-doc shard were 16 ms of the table's build (round 5 review, item 8)
    u32* d_long = nullptr;                                      // [n_terms] slot | [slices] term | [slices] slice | [n_long][BINS] hist | [n_long] max
    const u32 *d_slot = nullptr, *d_ghist = nullptr, *d_gmax = nullptr;
    {
        std::vector<u32> slot(ix->n_terms, 0xFFFFFFFFu), sl_term, sl_first;
        u32 n_long = 0;
        const u64 slice = (u64)std::max<long long>(64, sa_opt(ix->opts.topf_slice, (long long)SA_TOPF_SLICE));
        for (u32 t = 0; t < ix->n_terms; t++) {
            const u64 df = ix->h_tf_off[t + 1] - ix->h_tf_off[t];
            if (df < 4ull * slice) continue;
            slot[t] = n_long++;
            for (u64 sl = 0; sl * slice < df; sl++) { sl_term.push_back(t); sl_first.push_back((u32)sl); }
        }
        if (n_long) {
            const size_t words = (size_t)ix->n_terms + 2 * sl_term.size() + (size_t)n_long * SA_TOPF_BINS + n_long;
            if (hipMalloc(&d_long, words * sizeof(u32)) == hipSuccess) {
                u32* const d_st = d_long + ix->n_terms;
                u32* const d_sf = d_st + sl_term.size();
                u32* const d_h = d_sf + sl_term.size();
                bool ok = hipMemcpyAsync(d_long, slot.data(), slot.size() * sizeof(u32), hipMemcpyHostToDevice, ix->stream) == hipSuccess &&
                          hipMemcpyAsync(d_st, sl_term.data(), sl_term.size() * sizeof(u32), hipMemcpyHostToDevice, ix->stream) == hipSuccess &&
                          hipMemcpyAsync(d_sf, sl_first.data(), sl_first.size() * sizeof(u32), hipMemcpyHostToDevice, ix->stream) == hipSuccess &&
                          hipMemsetAsync(d_h, 0, ((size_t)n_long * SA_TOPF_BINS + n_long) * sizeof(u32), ix->stream) == hipSuccess;
                if (ok) {
                    hipLaunchKernelGGL(sa_k_topf_hist_long, dim3((u32)sl_term.size()), dim3(256), 0, ix->stream, (const u64*)im->d_imp, (const u64*)ix->d_tf_off,
                                       (const u32*)d_st, (const u32*)d_sf, (const u32*)d_long, d_h, d_h + (size_t)n_long * SA_TOPF_BINS, slice);
                    // (the copies above read pageable host vectors that die with this scope)
                    ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ix->stream) == hipSuccess;
                }
                if (ok) { d_slot = d_long; d_ghist = d_h; d_gmax = d_h + (size_t)n_long * SA_TOPF_BINS; }
                else { (void)hipGetLastError(); hipFree(d_long); d_long = nullptr; }
            } else (void)hipGetLastError();
        }
    }
    const u32 grid = ix->n_terms < 16384u ? ix->n_terms : 16384u;
    hipLaunchKernelGGL(sa_k_make_topf, dim3(grid), dim3(256), 0, ix->stream, (const u64*)im->d_imp, (const u64*)ix->d_tf_off, ix->n_terms, rk,
                       im->d_topf, im->d_maxf, d_slot, d_ghist, d_gmax);
    const bool topf_ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(ix->stream) == hipSuccess;
    if (d_long) hipFree(d_long);
    if (!topf_ok) {
        (void)hipGetLastError();
        hipFree(im->d_topf); im->d_topf = nullptr;
        if (im->d_maxf) { hipFree(im->d_maxf); im->d_maxf = nullptr; }
        return;
    }
    // host copies (the staged-tile route plans a query set on the host: starting bounds, score bounds of its terms)
    if (im->d_maxf) {
        im->h_topf.resize((size_t)ix->n_terms * SA_TOPF_NR);
        im->h_maxf.resize(ix->n_terms);
        if (hipMemcpy(im->h_topf.data(), im->d_topf, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(im->h_maxf.data(), im->d_maxf, (size_t)ix->n_terms * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            im->h_topf.clear(); im->h_maxf.clear();
        }
    }
}

// Saturation table of a batch, laid out [dl][tf - 1].  For integer doc lengths dl < tab_w and term frequencies
// 1 <= tf <= SA_SAT_NTF the per-posting factor  tf / (tf + k1 * ((1 - b) + b * (dl / avgdl)))
// depends only on (tf, dl) and the batch constants, so it is tabulated once per batch with the
// reference's exact operation order (bm25.pyx:19-23: every op rounded to fp32, IEEE division) and
// copied into LDS by each workgroup: scoring a posting becomes one LDS read and one multiply by
// idf instead of two divisions.  Postings outside the table take the arithmetic path.
#define SA_GRID_Y 32768u      // tiles per grid.y slab of the tile kernel's (queries, tiles) grid

__global__ void sa_k_make_sattab(float* __restrict__ tab, u32 tab_w, float k1, float b, float avgdl) {
    const float one_minus_b = 1.0f - b;
    const u32 n = SA_SAT_NTF * tab_w;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float tf = (float)(i % SA_SAT_NTF + 1), dl = (float)(i / SA_SAT_NTF);   // [dl][tf - 1]: index = dl << 3 | tf - 1
        const float norm = __fmul_rn(k1, __fadd_rn(one_minus_b, __fmul_rn(b, __fdiv_rn(dl, avgdl))));
        tab[i] = __fdiv_rn(tf, __fadd_rn(tf, norm));
    }
}

// Per-batch slice table: for every (query, term, tile) the first posting of that term whose
// doc id is >= tile * TILE, relative to the term's posting base (qbase).  Built once per batch
// (the index is immutable) from the tile directory -- or by a lower-bound search for terms too
// rare to have a directory row -- so the scoring kernel finds its slices with ONE dependent load.
__global__ void __launch_bounds__(256)
sa_k_make_bounds(const u64* __restrict__ tfp, const u64* __restrict__ tf_off, const u32* __restrict__ dir_slot,
                 const u32* __restrict__ tile_dir, u32 n_terms, u32 n_tiles, u32 tile_docs,
                 const u32* __restrict__ terms, u32 BT, u32* __restrict__ bounds, u64* __restrict__ qbase,
                 u64* __restrict__ qbase_imp, const float* __restrict__ topf, const float* __restrict__ idf, u32 T, u32 rank_idx,
                 u32* __restrict__ seed, float seed_scale) {
    const u64 total = (u64)BT * (n_tiles + 1);
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
        const u32 qt = (u32)(e / (n_tiles + 1)), tile = (u32)(e % (n_tiles + 1));
        const u32 term = terms[qt];
        u32 rel = 0;
        u64 base = 0, ibase = 0, isent = 0;
        if (term < n_terms) {
            base = tf_off[term];
            ibase = sa_imp_base(base, term);
            isent = sa_imp_sentinel(ibase, tf_off[term + 1] - base);
            const u32 cnt = (u32)(tf_off[term + 1] - base);
            const u32 slot = dir_slot[term];
            if (slot != 0xFFFFFFFFu) rel = tile_dir[(u64)slot * (n_tiles + 1) + tile];
            else rel = sa_lower_bound(tfp + base, 0, cnt, ((u64)tile * tile_docs) << SA_KEY_SHIFT, SA_KEY_MASK);
        }
        bounds[e] = rel;
        if (tile == 0) {
            qbase[qt] = base;
            if (qbase_imp) { qbase_imp[2 * (u64)qt] = ibase; qbase_imp[2 * (u64)qt + 1] = isent; }
            // the query's starting bound: the best of  weight x (k-th largest factor of the term, or of a rank beyond k)
            // over its terms (sa_impacts::d_topf; seed[] arrives zeroed with the upload)
            if (seed && term < n_terms) {
                // (seed_scale: 1.0 -- x * 1.0 = x bit for bit -- except under the test hook that forces bounds which are too high)
                const float s = __fmul_rn(__fmul_rn(topf[(u64)term * SA_TOPF_NR + rank_idx], idf[qt]), seed_scale);
                if (s > 0.f) atomicMax(&seed[qt / T], __float_as_uint(s));
            }
        }
    }
}

// MODE 0: dense output and/or block-level threshold top-k (any k <= 1024).
// MODE 1: pruned wave-level top-k against the query's global bound (any k <= 1024), the batch fast path.
// One work item = one (tile, query) pair; `qi` indexes the queries in play (p.qlist maps it, if set).
// IMP: read the impact stream (p.imp / p.qbase_imp) instead of the TF postings.  A batch of 8 postings per
// lane then updates its accumulators together -- 8 LDS reads in flight, the adds, 8 writes -- and a posting
// outside the tile is steered to a spare slot behind the tile instead of being branched around.
// LDS of one tile item: the accumulators (+ one spare slot per lane: acc[TILE + lane]) aliased with the
// MODE 0 selection lists, and the saturation table (TF route) / the selection's per-wave histogram scratch
// (impact route).  Declared by the kernels and handed to the item, so that a kernel which does other work
// on the same tile (sa_k_bm25_group_tiles) can lend the item its own accumulators.
template <int TILE, int MODE>
__host__ __device__ constexpr size_t sa_tile_smem_u64() {
    constexpr int CAP = (TILE >= 8192) ? 2048 : TILE / 4;
    constexpr size_t ACC_BYTES = (size_t)TILE * 4;
    constexpr size_t SEL_BYTES = MODE == 0 ? (size_t)(CAP + SA_KMAX) * 8 : 0;
    return (ACC_BYTES > SEL_BYTES ? ACC_BYTES : SEL_BYTES) / 8 + SA_WAVE / 2;
}
template <int THREADS, bool IMP>
__host__ __device__ constexpr int sa_tile_tab_floats() {
    constexpr int NW = THREADS / SA_WAVE;
    return IMP ? (NW * SA_HBINS / 2 > 64 ? NW * SA_HBINS / 2 : 64) : SA_SAT_NTF * SA_SAT_WMAX;
}

// MM: minimum-should-match (p.min_match_off, sa_batch_set_min_match).  The item keeps a byte per doc beside the accumulators (`mc`, TILE +
// one spare per lane -- shared by the waves, never read for a result --, handed in by the kernel like the accumulators): the number of query slots whose own product was > 0.  A tile in
// which fewer than m of the query's terms have postings is left before a posting is read; the accumulators of docs that matched fewer
// than m slots are cleared BEFORE the filter clear and any selection, so everything downstream is unchanged.  A term phase touches a
// doc at most once and phases are separated by barriers: the update is a plain byte read-modify-write (ds_read_u8 / ds_write_b8 --
// byte stores of different lanes into one dword do not disturb each other).  The instantiations without MM contain none of it.
// MM == 2: occur classes as well (p.occur_off, sa_batch_set_occur): every slot of the query is optional, required or prohibited, and m
// counts the optional ones.  The state per doc is 16 bits wide (SA_OCC_*): matched optional slots in bits 0-5, matched required slots in
// bits 6-11, bit 12 set by a prohibited slot -- a slot's class is uniform for its phase, so the update keeps the shape of the byte's.
// A prohibited slot is tested with its real product and not added at all (the same bits as adding it with weight 0: x + 0 is exact), so
// its phase leaves the accumulators alone.  Tiles that cannot hold a doc that passes
// are left like those of MM == 1; a doc stays when its state says  optional >= m, required == all of them, prohibited none.
#define SA_OCC_SHOULD 1u
#define SA_OCC_MUST 0x40u
#define SA_OCC_NOT 0x1000u
template <int MM> struct sa_match_state { typedef unsigned char type; };
template <> struct sa_match_state<2> { typedef unsigned short type; };
template <int TILE, int THREADS, int MODE, bool IMP, int MM = 0>
__device__ __forceinline__ void sa_bm25_tile_item(const Bm25Params& p, const u32 tile, const u32 qi, u64* smem, float* s_tab,
                                                  typename sa_match_state<MM>::type* mc = nullptr) {
    constexpr bool OCC = MM == 2;
    typedef typename sa_match_state<MM>::type mc_t;
    constexpr int NW = THREADS / SA_WAVE;
    constexpr int E = TILE / THREADS;
    constexpr int CAP = (TILE >= 8192) ? 2048 : TILE / 4;      // candidate list capacity (MODE 0)
    constexpr int LE = (CAP + THREADS - 1) / THREADS;
    constexpr int PF = 4;                                       // 16-byte loads in flight per lane
    __shared__ u64 red64[NW + 1];
    __shared__ u32 red[NW + 1];
    __shared__ u32 s_cnt[2];
    float* acc = (float*)smem;

    // Work items (tile, query) are dispatched tile-major, one workgroup per item: the items in
    // flight at any moment are the same few tiles across many queries, so posting slices shared
    // by queries are served from L2.  (Resident grids were measured slower on MI355X, twice: walking
    // the items with a static stride -- 3.3-3.7 ms vs 2.7 ms per 256-query batch at 10M docs -- and
    // pulling them from an atomic work queue with the next item's loads requested ahead -- 3.1 ms vs
    // 1.6 ms: DESIGN 3.1.)
    const u32 tid = threadIdx.x;
    const u32 T = p.T;
    const u32 tab_w = p.tab_w;
    if constexpr (!IMP) {
        for (u32 i = tid; i < SA_SAT_NTF * tab_w; i += THREADS) s_tab[i] = p.sattab[i];
    }
    // (queries answered by the sparse candidate path, sa_sparse.hip, are not in the list)
    const u32 q = p.qlist ? p.qlist[qi] : qi;
    const u64 tile_base = (u64)tile * TILE;
    // pruning slots of this query (see the top-k section); loaded first so the L2 latency hides
    // behind the posting stream.  L1-bypassing load: a fresher bound prunes more.
    // (k > 32 on tiles of <= 4 waves: the cached histogram bound instead, see sa_tile_topk_hist)
    constexpr bool HIST_OK = (size_t)NW * SA_HBINS * 2 <= sizeof(float) * SA_SAT_NTF * SA_SAT_WMAX;   // 16-bit bins (<= 8 waves)
    const bool use_hist = MODE == 1 && HIST_OK && p.hist != nullptr;
    u32 slot_val = 0xFFFFFFFFu;
    if (MODE == 1 && !use_hist && (tid & (SA_WAVE - 1)) < 32u)
        slot_val = __hip_atomic_load(&p.slots[q * 32u + (tid & 31u)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (use_hist) {
        slot_val = __hip_atomic_load(&p.gthr[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p.seed) { const u32 sd = p.seed[q]; slot_val = sd > slot_val ? sd : slot_val; }
    }

    // 1. this tile's slice [lo, hi) of every query term: one dependent load from the batch's slice
    //    table.  Lane t of EVERY wave requests term t's entries (the same few cache lines), so the
    //    slices reach the scalar registers by readlane -- no LDS staging, no barrier between the lookup
    //    and the first posting loads; the accumulators are cleared while those are in flight.
    const u32 lane = tid & (u32)(SA_WAVE - 1);
    u64 r_lo = 0, r_hi = 0, r_send = 0;                         // r_send: the sentinel pair behind the term (impact stream)
    float r_idf = 0.f;
    if (lane < T) {
        const u32 qt = q * T + lane;
        const u32* row = p.bounds + (u64)qt * (p.n_tiles + 1) + tile;
        u64 base;
        if constexpr (IMP) {
            const sa_u64x2 bs = ((const sa_u64x2*)p.qbase_imp)[qt];
            base = bs.x;
            r_send = bs.y;
        } else {
            base = p.qbase[qt];
        }
        const u32 r0 = row[0], r1 = row[1];
        r_lo = base + r0;
        r_hi = base + r1;
        r_idf = p.idf[qt];
    }
    // the query terms with postings in this tile: phases of the others are skipped altogether
    u32 todo = (u32)__ballot(r_hi > r_lo);
    if (p.filt) {                                               // (uniform) a tile without an eligible doc: as if no term had postings in it
        constexpr u32 NB = (u32)TILE / 1024u;                   // (the filter's summary blocks: 1024 docs, SA_FILTER_BLOCK)
        u32 any = 0;
        for (u32 i = 0; i < NB; i++) { const u32 bi = tile * NB + i; any |= bi < p.filt_nblk ? p.filt_blk[bi] : 0u; }
        if (!any) todo = 0u;
    }
    u32 mm = 0;                                                 // (uniform) slots a doc of this query must match
    u32 o_must = 0, o_not = 0, n_must = 0;                      // (uniform) the query's required / prohibited slots, MM == 2
    if constexpr (MM != 0) {
        mm = ((const u32*)((const char*)p.terms + p.min_match_off))[q];
        bool skip;
        if constexpr (OCC) {
            const u32* oc = (const u32*)((const char*)p.terms + p.occur_off) + 2u * q;
            o_must = oc[0]; o_not = oc[1];
            n_must = (u32)__builtin_popcount(o_must);
            // a required term without postings in this tile, fewer than mm optional ones with postings, or prohibited ones only
            skip = (todo & o_must) != o_must || (u32)__builtin_popcount(todo & ~(o_must | o_not)) < mm || (todo & ~o_not) == 0u;
        } else {
            // fewer than mm of the query's terms have postings in this tile: no doc of it can match mm slots
            skip = (u32)__builtin_popcount(todo) < mm;
        }
        if (todo != 0u && skip) {
            todo = 0u;
            if (p.stats && tid == 0) atomicAdd(&p.stats[q], 1u);
        }
    }
    // the state of a doc after a posting of a phase of class `cls` (SA_OCC_*; MM == 1: every slot counts one) whose product is `prod`
    auto bump = [](u32 c, float prod, u32 cls) -> u32 {
        if constexpr (OCC) return prod > 0.f ? ((c + (cls & (SA_OCC_NOT - 1u))) | (cls & SA_OCC_NOT)) : c;
        else return c + (prod > 0.f ? 1u : 0u);
    };
    // a phase's postings are added to the accumulators (uniform; not those of a prohibited slot)
    auto adds = [](u32 cls) -> bool { return cls != SA_OCC_NOT; };
    // the state beside the accumulator at byte offset s
    auto mc_at = [&](u32 s) -> mc_t& { return mc[s >> 2]; };
    auto lane64 = [](u64 x, u32 l) -> u64 {                      // value of lane l (wave-uniform l) in scalar registers
        const u32 a = (u32)__builtin_amdgcn_readlane((int)(u32)x, (int)l), b = (u32)__builtin_amdgcn_readlane((int)(u32)(x >> 32), (int)l);
        return ((u64)b << 32) | a;
    };

    // 2. term-at-a-time accumulation.  A slice is read as 16-byte pairs from its 16-byte-aligned
    //    hull (one global_load_dwordx4 per lane, PF in flight); a pair element outside [lo, hi)
    //    belongs to a neighbouring tile and is masked.  The first PF loads of term t+1 are issued
    //    before term t is scored, so short slices cost no extra memory round trip.
    const float k1 = p.k1, bb = p.b, avgdl = p.avgdl;
    const float one_minus_b = 1.0f - bb;
    // Per posting: unpack, saturation-table lookup (or the arithmetic path for out-of-table
    // tf / dl), multiply by idf, and a read-modify-write of the doc's LDS accumulator.  One
    // posting per (term, doc): no two lanes of a term phase touch the same slot.
    auto score_into = [&](u64 x, bool valid, float idf, u32 cls) {
        const u32 d = (u32)((x >> SA_KEY_SHIFT) - tile_base);
        const u32 tfi = (u32)(x & SA_LSB_MASK);
        const u32 dli = (u32)((x >> SA_LSB_BITS) & SA_LSB_MASK);
        if (valid) {
            float sat;
            if (tfi - 1u < (u32)SA_SAT_NTF && dli < tab_w) {
                sat = s_tab[(dli << 3) + tfi - 1u];              // [dl][tf - 1] (SA_SAT_NTF == 8): shift + add, no multiply
            } else {
                const float tf = (float)tfi;
                const float dl = p.dl_packed ? (float)dli : p.doc_lens[tile_base + d];
                const float norm = __fmul_rn(k1, __fadd_rn(one_minus_b, __fmul_rn(bb, __fdiv_rn(dl, avgdl))));
                sat = __fdiv_rn(tf, __fadd_rn(tf, norm));
            }
            const float prod = __fmul_rn(sat, idf);
            if constexpr (OCC) {
                if (adds(cls)) acc[d] = __fadd_rn(acc[d], prod);
            } else {
                acc[d] = __fadd_rn(acc[d], prod);
            }
            if constexpr (MM != 0) mc[d] = (mc_t)bump(mc[d], prod, cls);
        }
    };
    // Impact stream: the factor is in the posting and a posting is valid iff its doc lies in this tile
    // (terms start on even indices and gaps hold an all-ones sentinel, so whatever else a pair load of
    // the hull brings along -- the previous / next tile's posting, padding -- fails the same test).
    const u32 tile_base_b = (u32)tile_base * 4u;                // the stream holds doc * 4: byte offsets into the accumulators
    auto acc_at = [&](u32 byte_off) -> float& { return *(float*)((char*)acc + byte_off); };
    const u64* const stream = IMP ? p.imp : p.tfp;
    struct Batch { sa_u64x2 v[PF]; };
    // All indices below are relative to a0, the 16-byte-aligned start of the slice's hull: a slice is
    // far shorter than 2^32 postings, so the per-posting bookkeeping is 32-bit.
    // pairs [first, first + PF*THREADS) of the hull of [lo, hi)
    // `send` (impact stream): first cell of the sentinel pair behind the slice's term.  Every load of the
    // impact stream is unconditional and clamped to that pair: what lies between the end of the slice and
    // it are the term's postings of later tiles, which fail the doc test like the sentinels themselves --
    // no per-lane bounds test, no fill value, nothing to invalidate.
    auto load_batch = [&](u64 lo, u64 hi, u64 send, u32 first) -> Batch {
        Batch b;
        const u64 a0 = lo & ~1ull;
        const sa_u64x2* pairs = (const sa_u64x2*)(stream + a0);
        if constexpr (IMP) {
            const u32 jc = (u32)((send - a0) >> 1);
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const u32 j = first + (u32)u * THREADS + tid;
                b.v[u] = pairs[j < jc ? j : jc];
            }
        } else {
            const u32 npairs = (hi > a0) ? (u32)((hi - a0 + 1) >> 1) : 0u;
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const u32 j = first + (u32)u * THREADS + tid;
                if (j < npairs) b.v[u] = pairs[j];
                else { b.v[u].x = 0; b.v[u].y = 0; }
            }
        }
        return b;
    };
    // impact stream: one pair per lane
    auto score_pair = [&](const sa_u64x2& v, float idf, u32 cls) {
        const u32 spare = ((u32)TILE + (tid & (u32)(SA_WAVE - 1))) * 4u;
        const u32 d0 = (u32)(v.x >> 32) - tile_base_b, d1 = (u32)(v.y >> 32) - tile_base_b;
        const u32 s0 = d0 < (u32)TILE * 4u ? d0 : spare, s1 = d1 < (u32)TILE * 4u ? d1 : spare;
        if constexpr (OCC) {
            if (!adds(cls)) {                                   // (uniform) a prohibited slot: the states only
                const u32 c0 = mc_at(s0), c1 = mc_at(s1);
                mc_at(s0) = (mc_t)bump(c0, __fmul_rn(__uint_as_float((u32)v.x), idf), cls);
                mc_at(s1) = (mc_t)bump(c1, __fmul_rn(__uint_as_float((u32)v.y), idf), cls);
                return;
            }
        }
        const float v0 = acc_at(s0), v1 = acc_at(s1);
        const float p0 = __fmul_rn(__uint_as_float((u32)v.x), idf);
        const float w0 = __fadd_rn(v0, p0);
        const float p1 = __fmul_rn(__uint_as_float((u32)v.y), idf);
        const float w1 = __fadd_rn(v1, p1);
        acc_at(s0) = w0;
        acc_at(s1) = w1;
        if constexpr (MM != 0) {                                // (state s >> 2 beside accumulator s; a sentinel's product is NaN: not > 0)
            const u32 c0 = mc_at(s0), c1 = mc_at(s1);
            mc_at(s0) = (mc_t)bump(c0, p0, cls);
            mc_at(s1) = (mc_t)bump(c1, p1, cls);
        }
    };
    auto score_batch = [&](const Batch& b, u64 lo, u64 hi, u32 first, float idf, u32 cls) {
        const u64 a0 = lo & ~1ull;
        const u32 npairs = (hi > a0) ? (u32)((hi - a0 + 1) >> 1) : 0u;
        if constexpr (IMP) {
            const u32 spare = ((u32)TILE + (tid & (u32)(SA_WAVE - 1))) * 4u;
            if (first + (tid & ~(u32)(SA_WAVE - 1)) >= npairs) return;     // wave-uniform: no pair of this batch is this wave's
            if (npairs - first <= (u32)THREADS) {               // the last step of a slice (a short slice's only one)
                score_pair(b.v[0], idf, cls);
                return;
            }
            // lanes / steps past the end of the slice hold sentinels
            u32 slot[2 * PF];
            float val[2 * PF];
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const u32 d0 = (u32)(b.v[u].x >> 32) - tile_base_b, d1 = (u32)(b.v[u].y >> 32) - tile_base_b;
                slot[2 * u] = d0 < (u32)TILE * 4u ? d0 : spare;
                slot[2 * u + 1] = d1 < (u32)TILE * 4u ? d1 : spare;
            }
            // the same batch of eight on the match states, all reads before all writes as below -- and behind the accumulators'
            // stores, when the eight sums have left the registers (in front of them: 131 VGPRs, a wave per SIMD less)
            auto states = [&]() {
                u32 cnt[2 * PF];
#pragma unroll
                for (int i = 0; i < 2 * PF; i++) cnt[i] = mc_at(slot[i]);
#pragma unroll
                for (int u = 0; u < PF; u++) {
                    cnt[2 * u] = bump(cnt[2 * u], __fmul_rn(__uint_as_float((u32)b.v[u].x), idf), cls);
                    cnt[2 * u + 1] = bump(cnt[2 * u + 1], __fmul_rn(__uint_as_float((u32)b.v[u].y), idf), cls);
                }
#pragma unroll
                for (int i = 0; i < 2 * PF; i++) mc_at(slot[i]) = (mc_t)cnt[i];
            };
            if constexpr (OCC) {
                if (!adds(cls)) {                               // (uniform) a prohibited slot: the states only
                    states();
                    return;
                }
            }
#pragma unroll
            for (int i = 0; i < 2 * PF; i++) val[i] = acc_at(slot[i]);
#pragma unroll
            for (int u = 0; u < PF; u++) {
                val[2 * u] = __fadd_rn(val[2 * u], __fmul_rn(__uint_as_float((u32)b.v[u].x), idf));
                val[2 * u + 1] = __fadd_rn(val[2 * u + 1], __fmul_rn(__uint_as_float((u32)b.v[u].y), idf));
            }
#pragma unroll
            for (int i = 0; i < 2 * PF; i++) acc_at(slot[i]) = val[i];
            if constexpr (MM != 0) states();
            return;
        }
        const u32 r_lo = (u32)(lo - a0), r_hi = (u32)(hi - a0);     // the slice inside its hull
#pragma unroll
        for (int u = 0; u < PF; u++) {
            // wave-uniform skip: no lane of this wave has a pair at this step
            const u32 jw = first + (u32)u * THREADS + (tid & ~(u32)(SA_WAVE - 1));
            if (jw >= npairs) continue;
            const u32 r0 = 2u * (first + (u32)u * THREADS + tid);
            score_into(b.v[u].x, r0 >= r_lo && r0 < r_hi, idf, cls);
            score_into(b.v[u].y, r0 + 1u < r_hi, idf, cls);      // r0 + 1 >= r_lo always holds
        }
    };
    // Only terms with postings in this tile get a phase (and its barrier): an empty phase still costs
    // address arithmetic and a barrier -- measured 0.15 ms per term and launch at 10 M docs x 256
    // queries, more than the postings of the rare terms themselves.
    if (MODE == 1 && todo == 0u) return;                        // nothing scored: no doc can enter the top-k
    // Phases are taken in groups of four.  A group's prologue moves the slices (lo, hi, idf) of its
    // terms into scalar registers and requests the first 16 bytes per lane of ALL its phases (P[0..3]);
    // the rest of a phase's first batch -- only slices longer than one step have one -- is requested
    // one phase ahead (nxt).  Inside the group a phase starts from registers: a phase with few
    // postings (the rare terms of a query) otherwise spends far longer on address arithmetic and its
    // own memory round trip than on its postings (measured: 0.2 ms per term and
    // launch at 10 M docs x 256 queries, whatever the number of postings).
    auto load_step = [&](u64 lo, u64 hi, u64 send, u32 step) -> sa_u64x2 {     // step `step` of the first batch
        const u64 a0 = lo & ~1ull;
        const sa_u64x2* pairs = (const sa_u64x2*)(stream + a0);
        const u32 j = step * THREADS + tid;
        if constexpr (IMP) {
            const u32 jc = (u32)((send - a0) >> 1);
            return pairs[j < jc ? j : jc];
        } else {
            const u32 npairs = (hi > a0) ? (u32)((hi - a0 + 1) >> 1) : 0u;
            sa_u64x2 v;
            if (j < npairs) v = pairs[j];
            else { v.x = 0; v.y = 0; }
            return v;
        }
    };
    auto pairs_of = [](u64 lo, u64 hi) -> u32 {
        const u64 a0 = lo & ~1ull;
        return (hi > a0) ? (u32)((hi - a0 + 1) >> 1) : 0u;
    };
    // steps 1 .. PF-1 of a slice's first batch (nothing to fetch for a slice of one step)
    auto load_rest = [&](Batch& b, u64 lo, u64 hi, u64 send) {
        if (pairs_of(lo, hi) > (u32)THREADS) {
#pragma unroll
            for (int u = 1; u < PF; u++) b.v[u] = load_step(lo, hi, send, (u32)u);
        } else {
            const u64 fill = IMP ? ~0ull : 0ull;
#pragma unroll
            for (int u = 1; u < PF; u++) { b.v[u].x = fill; b.v[u].y = fill; }
        }
    };
    // The first loads of a group are UNCONDITIONAL (TF postings: lanes past the end of a slice re-read its last
    // pair and are zeroed when the pair is consumed) and issued in the order  first batch of phase 0, second
    // batch of phase 0 if its slice is long, first step of phases 1..3 : the compiler can then count them,
    // and phase 0 -- peeled out of the loop below -- waits with vmcnt(3) for its own data only.  The slices of
    // the rare terms (never shared between queries, so they come from HBM, not L2) arrive while the
    // frequent first term is being scored instead of holding the workgroup up before it starts.
    auto load_step_u = [&](u64 lo, u64 hi, u64 send, u32 step) -> sa_u64x2 {
        if constexpr (IMP) {
            return load_step(lo, hi, send, step);
        } else {
            const u64 a0 = lo & ~1ull;
            const u32 npairs = pairs_of(lo, hi);
            const sa_u64x2* pairs = (const sa_u64x2*)(stream + a0);
            const u32 j = step * THREADS + tid;
            const u32 last = npairs ? npairs - 1u : 0u;
            return pairs[j < last ? j : last];
        }
    };
    auto invalidate = [&](sa_u64x2& v, u32 j, u32 npairs) {
        if constexpr (!IMP) {
            if (j >= npairs) { v.x = 0; v.y = 0; }
        }
    };
    // one term phase: the first batch `cur`, then -- long slices -- the rest, `b` being the second batch (already requested)
    auto run_phase = [&](const Batch& cur, Batch& b, u64 lo, u64 hi, u64 send, float idf, u32 cls) {
        const u32 npairs = pairs_of(lo, hi);
        score_batch(cur, lo, hi, 0, idf, cls);
        if (npairs > (u32)PF * THREADS) {
            u32 first = (u32)PF * THREADS;
            while (first < npairs) {
                const u32 nf = first + (u32)PF * THREADS;
                Batch b2;
                if (nf < npairs) b2 = load_batch(lo, hi, send, nf);
                score_batch(b, lo, hi, first, idf, cls);
                if (nf < npairs) b = b2;
                first = nf;
            }
        }
    };
    bool cleared = false;
    while (todo) {
        u64 L[4], H[4], S[4];
        float W[4];
        u32 C[4] = {SA_OCC_SHOULD, SA_OCC_SHOULD, SA_OCC_SHOULD, SA_OCC_SHOULD};     // the phases' classes (MM == 2; else never read)
        sa_u64x2 P[4];
        {
            u32 g = todo;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const bool have = g != 0u;
                const u32 ti = have ? (u32)__builtin_ctz(g) : 0u;
                g &= g - 1u;                                     // (0 stays 0)
                L[i] = have ? lane64(r_lo, ti) : 0ull;
                H[i] = have ? lane64(r_hi, ti) : 0ull;
                S[i] = (IMP && have) ? lane64(r_send, ti) : 0ull;
                W[i] = __uint_as_float((u32)__builtin_amdgcn_readlane((int)__float_as_uint(r_idf), (int)ti));
                if constexpr (OCC) C[i] = ((o_not >> ti) & 1u) ? SA_OCC_NOT : ((o_must >> ti) & 1u) ? SA_OCC_MUST : SA_OCC_SHOULD;
            }
        }
        // ---- phase 0 of the group
        {
            const u64 lo = L[0], hi = H[0];
            const u32 npairs = pairs_of(lo, hi);
            Batch cur, b;
#pragma unroll
            for (int u = 0; u < PF; u++) cur.v[u] = load_step_u(lo, hi, S[0], (u32)u);
            if (npairs > (u32)PF * THREADS) b = load_batch(lo, hi, S[0], (u32)PF * THREADS);
#pragma unroll
            for (int i = 1; i < 4; i++) P[i] = load_step_u(L[i], H[i], S[i], 0);
            if (!cleared) {                                     // first group: clear the accumulators behind the loads
#pragma unroll
                for (int j = 0; j < E; j++) acc[j * THREADS + tid] = 0.f;
                if constexpr (MM != 0) {                        // ... and the match states, a dword per store
#pragma unroll
                    for (int j = 0; j < E * (int)sizeof(mc_t) / 4; j++) ((u32*)mc)[j * THREADS + tid] = 0u;
                }
                __syncthreads();
                cleared = true;
            }
            todo &= todo - 1u;
#pragma unroll
            for (int u = 0; u < PF; u++) invalidate(cur.v[u], (u32)u * THREADS + tid, npairs);
            run_phase(cur, b, lo, hi, S[0], W[0], C[0]);
            __syncthreads();
        }
        // ---- phases 1..3
        if constexpr (IMP) {
            // Usual case: every further term of the group has a slice of one step (at most THREADS pairs).
            // Such a phase is its pair from P[k], one LDS update and the barrier -- none of the generic
            // phase's bookkeeping, which costs more than the update itself (measured: 0.14 ms per phase and
            // launch at 10 M docs x 256 queries for the generic loop).
            const u32 np1 = pairs_of(L[1], H[1]), np2 = pairs_of(L[2], H[2]), np3 = pairs_of(L[3], H[3]);
            if (np1 <= (u32)THREADS && np2 <= (u32)THREADS && np3 <= (u32)THREADS) {
                const u32 npk[4] = {0u, np1, np2, np3};
#pragma unroll
                for (int k = 1; k < 4; k++) {
                    if (npk[k] == 0u) break;                    // (absent terms are the last ones of a group)
                    todo &= todo - 1u;
                    if ((tid & ~(u32)(SA_WAVE - 1)) < npk[k]) {
                        sa_u64x2 v = P[k];
                        invalidate(v, tid, npk[k]);
                        score_pair(v, W[k], C[k]);
                    }
                    __syncthreads();
                }
                continue;
            }
        }
        Batch nxt;
        load_rest(nxt, L[1], H[1], S[1]);
#pragma unroll 1
        for (int k = 1; k < 4 && todo; k++) {
            todo &= todo - 1u;
            L[0] = L[1]; L[1] = L[2]; L[2] = L[3]; L[3] = 0;
            H[0] = H[1]; H[1] = H[2]; H[2] = H[3]; H[3] = 0;
            S[0] = S[1]; S[1] = S[2]; S[2] = S[3]; S[3] = 0;
            W[0] = W[1]; W[1] = W[2]; W[2] = W[3];
            C[0] = C[1]; C[1] = C[2]; C[2] = C[3];
            P[0] = P[1]; P[1] = P[2]; P[2] = P[3];
            const u64 lo = L[0], hi = H[0];
            const u32 npairs = pairs_of(lo, hi);
            Batch cur = nxt, b;
            cur.v[0] = P[0];
            invalidate(cur.v[0], tid, npairs);
            load_rest(nxt, L[1], H[1], S[1]);                   // (the next group's first phase: nothing, L[1] = H[1] = 0)
            if (npairs > (u32)PF * THREADS) b = load_batch(lo, hi, S[0], (u32)PF * THREADS);   // requested before the first batch is scored
            run_phase(cur, b, lo, hi, S[0], W[0], C[0]);
            __syncthreads();
        }
    }
    if (!cleared) {                                             // MODE 0 without any posting in the tile: all zero
#pragma unroll
        for (int j = 0; j < E; j++) acc[j * THREADS + tid] = 0.f;
        __syncthreads();
    }

    const u64 remain = p.n_docs - tile_base;
    const u32 tile_n = remain < (u64)TILE ? (u32)remain : (u32)TILE;
    // minimum-should-match: a doc that matched fewer than mm slots leaves the ranking here, like a filtered one below (a tile without
    // a scored posting holds zeros only, and its counts were never cleared)
    if constexpr (MM != 0) {
        if (cleared && (OCC || mm > 1u)) {                      // (uniform; with occur classes m <= 1 is a test too)
#pragma unroll
            for (int j = 0; j < E; j++) {
                const u32 e = j * THREADS + tid;
                const u32 c = mc[e];
                // (bits 6 and up: the required slots matched, and nothing above them -- no prohibited slot matched)
                if (OCC ? ((c & (SA_OCC_MUST - 1u)) < mm || (c >> 6) != n_must) : (c < mm)) acc[e] = 0.f;
            }
            __syncthreads();
        }
    }
    // the batch's document filter: the scores of the non-eligible docs are cleared BEFORE any selection, so that no excluded doc
    // ever raises a slot, a histogram bin or the cached bound, or becomes a candidate
    if (p.filt) {                                               // (uniform)
#pragma unroll
        for (int j = 0; j < E; j++) {
            const u32 e = j * THREADS + tid;
            const u64 w = e < tile_n ? p.filt[(tile_base + e) >> 6] : 0ull;
            if (!((w >> (e & 63u)) & 1ull)) acc[e] = 0.f;
        }
        __syncthreads();
    }

    // 3. dense drop-in output (SearchArray.score): coalesced tile store
    if (MODE == 0 && p.dense_out) {
        float* out = p.dense_out + (u64)q * p.n_docs + tile_base;
#pragma unroll
        for (int j = 0; j < E; j++) {
            const u32 e = j * THREADS + tid;
            if (e < tile_n) out[e] = acc[e];
        }
    }
    const u32 k = p.k;
    if (p.cand && !p.no_topk) {
    if constexpr (MODE == 1) {
        if constexpr (HIST_OK) {
            if (use_hist) {
                // the saturation table is dead (barrier after the last term): its LDS is the waves' scratch
                sa_tile_topk_hist<TILE, THREADS>(acc, slot_val, q, tile, p.doc_base + tile_base, k, p.hist, p.gthr, p.cand,
                                                 p.cand_cap, p.cand_cnt, (u32*)s_tab);
                return;
            }
        }
        sa_tile_topk_pruned<TILE, THREADS>(acc, slot_val, q, tile, p.doc_base + tile_base, k, p.slots, p.cand,
                                           p.cand_cap, p.cand_cnt);
    } else {
    // 4. per-tile top-k -> composite keys  score_bits<<32 | ~global_doc
    u64* cand = p.cand + ((u64)q * p.n_tiles + tile) * p.cand_per_tile;
    u64* sel = smem + CAP;                    // selected keys (aliases acc once keys are in registers)
    u32 nsel = 0;
    // general k: threshold selection.
    u32 key32[E];
    u32 lmax = 0, nnz_local = 0;
#pragma unroll
    for (int j = 0; j < E; j++) {
        key32[j] = __float_as_uint(acc[j * THREADS + tid]);
        lmax = key32[j] > lmax ? key32[j] : lmax;
        nnz_local += key32[j] != 0 ? 1u : 0u;
    }
    if (tid == 0) { s_cnt[0] = 0; s_cnt[1] = 0; }
    const u32 nnz = sa_block_sum<NW>(nnz_local, red);            // barriers: acc is dead from here on
    if (nnz > 0) {
        u32 theta = 1;
        if (nnz > k && k <= (u32)THREADS) {
            // k-th largest per-thread maximum is a lower bound of the tile's k-th largest score
            const u64 th = sa_block_kth_largest<1, NW>([&](int) { return (u64)lmax; }, k, red64);
            theta = th > 1 ? (u32)th : 1u;
        }
        u32 c_local = 0;
#pragma unroll
        for (int j = 0; j < E; j++) c_local += key32[j] >= theta ? 1u : 0u;
        const u32 C = sa_block_sum<NW>(c_local, red);
        if (C <= (u32)CAP) {
            // gather the survivors into an LDS list, then select exactly among them
            u64* list = smem;
#pragma unroll
            for (int j = 0; j < E; j++) {
                if (key32[j] >= theta) {
                    const u32 pos = atomicAdd(&s_cnt[0], 1u);
                    list[pos] = ((u64)key32[j] << 32) | (u64)(0xFFFFu - (u32)(j * THREADS + tid));
                }
            }
            __syncthreads();
            u64 lk[LE];
#pragma unroll
            for (int e = 0; e < LE; e++) {
                const u32 idx = e * THREADS + tid;
                lk[e] = idx < C ? list[idx] : 0ull;
            }
            u64 kth = 1;
            if (C > k) kth = sa_block_kth_largest<LE, NW>([&](int e) { return lk[e]; }, k, red64);
#pragma unroll
            for (int e = 0; e < LE; e++) {
                if (lk[e] != 0 && lk[e] >= kth) {
                    const u32 pos = atomicAdd(&s_cnt[1], 1u);
                    if (pos < (u32)SA_KMAX) sel[pos] = lk[e];
                }
            }
        } else {
            // Too many survivors (massive ties).  Rare: bisect over the score bits still sitting in
            // the LDS tile (re-read every step -- slow but register-free), composite keys formed on
            // the fly; `sel` aliases part of the tile, so winners are staged through `list` slots
            // only after the last read.
            const u32* tile_bits = (const u32*)smem;
            u64 m = 0;
            for (int j = 0; j < E; j++) {
                const u32 e = j * THREADS + tid;
                const u32 kb = tile_bits[e];
                const u64 c = kb ? (((u64)kb << 32) | (u64)(0xFFFFu - e)) : 0ull;
                m = c > m ? c : m;
            }
            m = sa_block_max64<NW>(m, red64);
            int top = 63 - __clzll((long long)m);
            if ((top & 1) == 0) top++;
            u64 prefix = 0;
            for (int bit = top; bit >= 1; bit -= 2) {
                const u64 c1 = prefix | (1ull << (bit - 1)), c2 = prefix | (2ull << (bit - 1)), c3 = prefix | (3ull << (bit - 1));
                u64 packed = 0;
                for (int j = 0; j < E; j++) {
                    const u32 e = j * THREADS + tid;
                    const u32 kb = tile_bits[e];
                    const u64 x = kb ? (((u64)kb << 32) | (u64)(0xFFFFu - e)) : 0ull;
                    packed += (x >= c1 ? 1ull : 0ull) + (x >= c2 ? (1ull << 21) : 0ull) + (x >= c3 ? (1ull << 42) : 0ull);
                }
#pragma unroll
                for (int o = SA_WAVE / 2; o > 0; o >>= 1) packed += __shfl_xor(packed, o, SA_WAVE);
                if (sa_lane() == 0) red64[sa_wave_id()] = packed;
                __syncthreads();
                u64 tot = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) tot += red64[w];
                __syncthreads();
                const u32 n1 = (u32)(tot & 0x1FFFFF), n2 = (u32)((tot >> 21) & 0x1FFFFF), n3 = (u32)((tot >> 42) & 0x1FFFFF);
                if (n3 >= k) prefix = c3; else if (n2 >= k) prefix = c2; else if (n1 >= k) prefix = c1;
            }
            const u64 thr = prefix > 1 ? prefix : 1;
            // every thread finished reading the tile (barrier above); now it may be overwritten
#pragma unroll
            for (int j = 0; j < E; j++) {
                const u32 e = j * THREADS + tid;
                const u64 c = key32[j] ? (((u64)key32[j] << 32) | (u64)(0xFFFFu - e)) : 0ull;
                if (c >= thr) {
                    const u32 pos = atomicAdd(&s_cnt[1], 1u);
                    if (pos < (u32)SA_KMAX) sel[pos] = c;
                }
            }
        }
    }
    __syncthreads();
    nsel = s_cnt[1] < k ? s_cnt[1] : k;
    for (u32 i = tid; i < p.cand_per_tile; i += THREADS) {
        u64 o = 0;
        if (i < nsel) {
            const u64 c = sel[i];
            const u64 doc = p.doc_base + tile_base + (0xFFFFu - (u32)(c & 0xFFFFu));
            o = (c & 0xFFFFFFFF00000000ull) | (u64)(u32)(~(u32)doc);
        }
        cand[i] = o;
    }
    }
    }   // top-k
}

// MM (minimum-should-match; 2: with occur classes): the match states, one or two bytes per accumulator and spare slot, lie BEHIND the item's LDS (the MODE 0 selection
// lists alias the accumulators, not the counts -- which are dead by then anyway)
template <int TILE, int THREADS, int MODE, bool IMP, int MM = 0>
__global__ void __launch_bounds__(THREADS) sa_k_bm25_tiles(const Bm25Params p) {
    // grid (queries, tiles): x runs fastest, so the dispatch order is tile-major without a division
    constexpr size_t ITEM_U64 = sa_tile_smem_u64<TILE, MODE>();
    typedef typename sa_match_state<MM>::type mc_t;
    __shared__ alignas(16) u64 smem[ITEM_U64 + (MM ? (TILE + SA_WAVE) * sizeof(mc_t) / 8 : 0)];
    __shared__ float s_tab[sa_tile_tab_floats<THREADS, IMP>()];
    const u32 tile = p.tile0 + blockIdx.z * SA_GRID_Y + blockIdx.y;
    if (tile >= p.tile_end) return;
    if constexpr (MM != 0) sa_bm25_tile_item<TILE, THREADS, MODE, IMP, MM>(p, tile, blockIdx.x, smem, s_tab, (mc_t*)(smem + ITEM_U64));
    else sa_bm25_tile_item<TILE, THREADS, MODE, IMP>(p, tile, blockIdx.x, smem, s_tab);
}

// The queries the sparse candidate path handed back (usually none): their number is only known on the
// device, so a resident grid walks the (tile, query) items of the list -- no host round trip to size a
// launch.  Slower per item than one workgroup per item, which does not matter for a rare fallback.
template <int TILE, int THREADS, bool IMP>
__global__ void __launch_bounds__(THREADS) sa_k_bm25_tiles_list(const Bm25Params p) {
    __shared__ alignas(16) u64 smem[sa_tile_smem_u64<TILE, 1>()];
    __shared__ float s_tab[sa_tile_tab_floats<THREADS, IMP>()];
    const u32 nq = *p.nq_dev;
    const u64 n_items = (u64)nq * p.n_tiles;
    for (u64 item = blockIdx.x; item < n_items; item += gridDim.x) {
        sa_bm25_tile_item<TILE, THREADS, 1, IMP>(p, (u32)(item / nq), (u32)(item % nq), smem, s_tab);
        __syncthreads();                              // LDS is reused by the next item
    }
}

// Facet counts (sa_batch_facet_counts, Part 2d): the tile item with a histogram where the selection is.  One workgroup per
// (tile, query), the grid of sa_k_bm25_tiles.  The item runs in MODE 0 over the TF postings with neither candidates nor a dense
// output: it returns behind the minimum-should-match clear and the filter clear, with the tile's final scores in LDS -- exactly the
// documents that can rank are > 0 -- and a barrier as its last act.  Every thread then walks its E documents: it counts those
// with a score > 0, reads their category codes (consecutive lanes read consecutive codes) and bumps a bin -- of a workgroup-private
// LDS histogram for columns of up to SA_FACET_LDS_BINS values, which ALIASES the saturation table (dead behind the last term phase,
// as sa_tile_topk_hist reuses it: 1024 u32 bins at no extra LDS) and is flushed with one global atomic per non-zero bin; of the
// query's row of the global counters directly for larger columns.  found / missing: a block sum and one atomic each.
// An item the tile item's own tests leave (no postings in the tile, an empty filter block, fewer than m terms present, a must term
// absent) holds zeros only: it finds nothing and returns without touching global memory.  Integer atomics: the result does not depend
// on their order.  The copy of the parameters with cand / dense_out / stats nulled lets the compiler drop the item's selection code.
// LDS of an item: the accumulators + spare slots (TILE x 4 + 256 bytes: no selection lists), the match states (MM), the table.
template <int TILE, int THREADS, int MM>
__global__ void __launch_bounds__(THREADS) sa_k_bm25_facet_tiles(const Bm25Params p_in, const FacetParams fp) {
    constexpr size_t ITEM_U64 = sa_tile_smem_u64<TILE, 1>();
    constexpr int NW = THREADS / SA_WAVE;
    constexpr int E = TILE / THREADS;
    static_assert(E <= 32, "a thread's documents fit a 32-bit mask");
    static_assert((u32)sa_tile_tab_floats<THREADS, false>() >= SA_FACET_LDS_BINS, "the LDS histogram aliases the saturation table");
    typedef typename sa_match_state<MM>::type mc_t;
    __shared__ alignas(16) u64 smem[ITEM_U64 + (MM ? (TILE + SA_WAVE) * sizeof(mc_t) / 8 : 0)];
    __shared__ float s_tab[sa_tile_tab_floats<THREADS, false>()];
    __shared__ u32 f_red[NW + 1];
    __shared__ u32 f_miss;
    const u32 tile = p_in.tile0 + blockIdx.z * SA_GRID_Y + blockIdx.y;
    if (tile >= p_in.tile_end) return;
    Bm25Params p = p_in;
    p.cand = nullptr; p.dense_out = nullptr; p.stats = nullptr; p.qlist = nullptr;
    const u32 q = blockIdx.x;
    if constexpr (MM != 0) sa_bm25_tile_item<TILE, THREADS, 0, false, MM>(p, tile, q, smem, s_tab, (mc_t*)(smem + ITEM_U64));
    else sa_bm25_tile_item<TILE, THREADS, 0, false>(p, tile, q, smem, s_tab);
    // (the item's last act is a barrier: the scores are final and the table is dead)
    const u32 tid = threadIdx.x;
    const float* const acc = (const float*)smem;
    const u64 tile_base = (u64)tile * TILE;
    const u64 remain = p.n_docs - tile_base;
    const u32 tile_n = remain < (u64)TILE ? (u32)remain : (u32)TILE;
    u32 mine = 0;                                               // bit j: document j * THREADS + tid of the tile matched
#pragma unroll
    for (int j = 0; j < E; j++) {
        const u32 e = j * THREADS + tid;
        if (e < tile_n && acc[e] > 0.f) mine |= 1u << j;
    }
    const u32 n_found = sa_block_sum<NW>((u32)__popc(mine), f_red);
    if (n_found == 0u) return;                                  // (uniform) nothing matched: no global access
    const u32 row = fp.row[q];
    if (!fp.codes) {                                            // (uniform) found only
        if (tid == 0) atomicAdd(&fp.found[row], n_found);
        return;
    }
    const u32 nv = fp.n_values;
    const bool lds = nv <= SA_FACET_LDS_BINS;                   // (uniform)
    u32* const bins = (u32*)s_tab;
    u32* const grow = fp.counts + (u64)row * nv;
    if (lds) for (u32 i = tid; i < nv; i += THREADS) bins[i] = 0u;
    if (tid == 0) f_miss = 0u;
    __syncthreads();
    u32 miss = 0;
#pragma unroll
    for (int j = 0; j < E; j++) {
        if ((mine >> j) & 1u) {
            const int c = fp.codes[tile_base + (u32)(j * THREADS) + tid];
            if (c < 0) miss++;
            else if (lds) atomicAdd(&bins[c], 1u);
            else atomicAdd(&grow[c], 1u);
        }
    }
    miss = sa_wave_sum(miss);
    if (sa_lane() == 0 && miss) atomicAdd(&f_miss, miss);
    __syncthreads();
    if (lds) {
        for (u32 i = tid; i < nv; i += THREADS) {
            const u32 c = bins[i];
            if (c) atomicAdd(&grow[i], c);
        }
    }
    if (tid == 0) {
        atomicAdd(&fp.found[row], n_found);
        if (f_miss) atomicAdd(&fp.missing[row], f_miss);
    }
}

// ---------------------------------------------------------------------------------------------
// Grouped exhaustive scoring: queries of a batch that share their FIRST term.
//
// Real batches repeat their frequent terms (the BASELINE query set draws its first term from ten terms),
// and the frequent term is where the postings are: per (tile, query) item of sa_k_bm25_tiles ~87 % of the
// posting loads and LDS updates belong to a term that 25 other queries of the batch score identically --
// same impact stream, same idf, and, the term being FIRST in query order, the same partial sum
// 0 + s0 = s0.  Here ONE wave owns a (tile, group) item:
//   base      the shared first term is scored once into the tile's accumulators ("base");
//   overlay   the queries of the group are taken one after the other: the postings of a query's further
//             terms are added IN PLACE in query-term order (so a doc's sum is ((s0 + s1) + s2) + s3 bit for
//             bit), the written value carrying its sign bit as a "touched by this query" mark; the lane that
//             touched a doc first evaluates the doc's final score against the query's bound, appends it
//             if it survives, and puts the base value back.  Docs a query does not touch score exactly the
//             base value: they need no per-query work at all as long as the tile's largest base value is
//             below the query's bound (else the general path below runs);
//   general   a query whose further terms have more postings in the tile than the overlay holds in registers,
//             or whose bound is not above the base values yet, is left to the per-query item: the (tile, query)
//             pair goes on a work list that sa_k_bm25_tiles_wl walks right after this kernel.
// Every posting of every query term is still read and scored -- nothing is skipped on a score bound; the
// shared term is read once per group instead of once per query.  Results are bit-identical to the per-query
// kernel (same candidates above the same bounds, same merge).  The next query's postings and bound are
// requested before the current one is processed (fixed number of loads per query, so the compiler can
// count them and wait for the current query's data only).
// ---------------------------------------------------------------------------------------------
#define SA_GRP_NH 10        // 64-posting halves of a query's further terms held in registers (640 postings per tile and query)

struct GroupParams {
    const u32* grp;         // [n_groups][3]: first device row, number of rows (rows of a group are contiguous), dense factor row of the shared first term or 0xFFFFFFFF
    const float* dense;     // dense factor rows (sa_impacts::d_dense), or null
    u64 dense_stride;
    u32 n_groups;
    u32 tile0, n_tiles_run; // tiles [tile0, tile0 + n_tiles_run)
    u32 tpx;                // tiles per XCD: XCD x takes the RANGE [x * tpx, (x + 1) * tpx) of the run's tiles (0: tiles t = x mod 8)
    u32 tt, tt_shift;       // lanes per query while the step tables are built: power of two >= max(T - 1, 1)
    u32 cq;                 // queries per table pass: an item of more queries builds its tables pass after pass over ONE base
    u64* wl;                // work list of (tile << 32 | device row) items left to the per-query kernel
    u32* wl_cnt;
};

// One HALF = up to 64 postings of ONE term of one query in this tile, one per lane (8-byte loads): every LDS
// instruction of the overlay touches the postings of a single term, i.e. pairwise distinct docs.  Its descriptor is
// ONE 8-byte LDS cell:
//   [47:0]  address of the half's first posting (impact stream)
//   [53:48] lim: the half's last posting; lane L loads posting min(L, lim).  The lanes past the half's postings so
//           hold COPIES of its last posting, and copies are harmless in a read-modify-write of one LDS instruction:
//           all of them read the same value, write the same value and later put the same value back -- the overlay
//           needs no per-lane validity test (the rare evaluation below does: a doc must be reported once)
//   [58:54] which of the query's overlaid terms (its weight sits in the item's weight table at [query][term])
//   [63:60] entry 0 of a query only: its number of halves (15: more than the table holds -> per-query kernel)
// (round 2 kept 16-byte entries with the weight inside: 3 KiB of table; with 8-byte entries, a 256 / 512-byte weight
//  table and a 32-entry survivor buffer an item needs 10 KiB of LDS -- 16 waves per CU instead of 12.)
#define SA_GRPH_LIM_SHIFT 48
#define SA_GRPH_TERM_SHIFT 54
#define SA_GRPH_NH_SHIFT 60
#define SA_GRPH_OVER 15u

// f(0), f(STEP), f(2 STEP), ... while the index is below n (< NH): nested tests, so the chain is left at the first
// index that is not, and every index is a compile-time constant (arrays indexed by it stay in registers)
template <int H, int NH, int STEP, class F>
__device__ __forceinline__ void sa_static_while_below(u32 n, F&& f) {
    if constexpr (H < NH) {
        if ((u32)H < n) {
            f(std::integral_constant<int, H>{});
            sa_static_while_below<H + STEP, NH, STEP>(n, f);
        }
    }
}

// s_waitcnt with vmcnt = 0 and the other counters open (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[15:14])
#define SA_WAIT_VMCNT0() __builtin_amdgcn_s_waitcnt(0x0F70)

#define SA_GRP_REFRESH_STEP 32
#define SA_GRP_SURV_CAP 32          // survivors an item buffers before it writes them out (a pair has at most 16)

// -DSA_PROBE (scripts/build_probe.sh; never in the product build): where a wave of the grouped kernel spends its cycles --
// s_memtime at the section boundaries, summed over the items that reach the overlay, read by sa_debug_probe_read.  Reading
// the clock waits for the wave's LDS operations (lgkmcnt(0)): sections that end with LDS writes are charged their drain.
#ifdef SA_PROBE
#define SA_PROBE_SLOTS 4096
__device__ unsigned long long g_sa_probe[SA_PROBE_SLOTS * 16];       // (slot = block mod SLOTS: no two waves in flight share cells)
#define SA_PT(i) do { const u64 t_ = __builtin_amdgcn_s_memtime(); pacc[i] += t_ - plast; plast = t_; } while (0)
#ifdef SA_PROBE_FINE      // sub-sections of the item's preamble: vector loads are waited for where they are charged
#define SA_PTV(i) do { __builtin_amdgcn_s_waitcnt(0x0F70); SA_PT(i); } while (0)
#else
#define SA_PTV(i) do { } while (0)
#endif
extern "C" int sa_debug_probe_read(unsigned long long* out16, int clear) {
    if (hipDeviceSynchronize() != hipSuccess) return SA_ERR_HIP;
    std::vector<unsigned long long> h((size_t)SA_PROBE_SLOTS * 16, 0ull);
    if (hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_sa_probe), h.size() * 8) != hipSuccess) return SA_ERR_HIP;
    for (int i = 0; i < 16; i++) { out16[i] = 0; for (int sl = 0; sl < SA_PROBE_SLOTS; sl++) out16[i] += h[(size_t)sl * 16 + i]; }
    if (clear) { std::fill(h.begin(), h.end(), 0ull); if (hipMemcpyToSymbol(HIP_SYMBOL(g_sa_probe), h.data(), h.size() * 8) != hipSuccess) return SA_ERR_HIP; }
    return SA_OK;
}
#else
#define SA_PT(i) do { } while (0)
#define SA_PTV(i) do { } while (0)
#endif

// IDFN: cells of the item's weight table = queries x lanes-per-query of the table build (64: up to 4 overlaid terms per
// query -- the BASELINE shape --, 128: anything else the host admits, n * tt <= 128)
// FILT: the batch has a document filter (sa_filter.hpp).  A tile without an eligible doc is left at once; the BASE cells of the
// non-eligible docs are cleared (so base_max -- what every untouched doc scores at most -- speaks of eligible docs only); and since
// the overlay adds to excluded docs as well (loose groups have no base at all), a doc's filter bit is part of the test that makes
// it a survivor: no excluded doc reaches a candidate list or a histogram.  Pairs left to the per-query kernel find the filter
// there.  The unfiltered instantiations contain none of it.
template <int TILE, int IDFN, bool FILT>
__global__ void __launch_bounds__(64, 4) sa_k_bm25_group_tiles(const Bm25Params p, const GroupParams gp) {
    constexpr int NH = SA_GRP_NH;
    static_assert(NH < (int)SA_GRPH_OVER && NH >= 8, "half count field");
    __shared__ alignas(16) u64 smem[sa_tile_smem_u64<TILE, 1>()];
    __shared__ u64 s_half[SA_GRP_MAXQ][NH];
    __shared__ float s_idf[IDFN];
    __shared__ u64 s_surv[SA_GRP_SURV_CAP];                     // survivors waiting for their places: score bits << 32 | accumulator offset << 6 | query of the item
    u32* const accu = (u32*)smem;
    const u32 lane = threadIdx.x;
#ifdef SA_PROBE
    u64 pacc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    u64 plast = __builtin_amdgcn_s_memtime();
#endif
    // XCD-aware item order: consecutive blocks go to consecutive XCDs (block b runs on XCD b % 8), so the
    // eight tiles of a chunk sit on eight XCDs and ALL groups of a tile follow each other on the same XCD:
    // the slices of the further terms that queries of different groups share are fetched into one L2 only.
    const u32 per = 8u * gp.n_groups;
    const u32 chunk = blockIdx.x / per, r = blockIdx.x % per;
    const u32 g = r >> 3;
    // ... and an XCD walks a RANGE of consecutive tiles: a term's slices of neighbouring tiles are neighbours in memory, and
    // with tiles dealt round-robin the cache line a tile's slice shares with the next tile's was fetched into two L2s -- for a
    // sparse term (4 postings = 32 bytes per tile) every line into four.
    const u32 trel = gp.tpx ? (r & 7u) * gp.tpx + chunk : chunk * 8u + (r & 7u);
    if (trel >= gp.n_tiles_run) return;
    const u32 tile = gp.tile0 + trel;
    if constexpr (FILT) {
        constexpr u32 NB = (u32)TILE / 1024u;                   // (the filter's summary blocks: 1024 docs)
        u32 any = 0;
        for (u32 i = 0; i < NB; i++) { const u32 bi = tile * NB + i; any |= bi < p.filt_nblk ? p.filt_blk[bi] : 0u; }
        if (!any) return;                                       // (uniform) nothing eligible in this tile
    }
    // a LOOSE group (bit 31 of the size): queries that share nothing -- no base, ALL their terms are overlaid on
    // cleared accumulators (0 + s0 = s0, so the sums are the same); what they share is the item's fixed cost
    const u32 row0 = gp.grp[3 * g], n_raw = gp.grp[3 * g + 1], n = n_raw & 0x7FFFFFFFu;
    const u32 dslot = gp.dense ? gp.grp[3 * g + 2] : 0xFFFFFFFFu;
    const bool loose = (n_raw >> 31) != 0u;
    const u32 T = p.T;
    const u64 tile_base = (u64)tile * TILE;
    const u32 tile_base_b = (u32)tile_base * 4u;
    const u32 spare = ((u32)TILE + lane) * 4u;                  // byte offset of this lane's spare slot
    const u64* const stream = p.imp;
    auto at = [&](u32 byte_off) -> u32& { return *(u32*)((char*)accu + byte_off); };
    auto ballot = [](bool c) -> u64 { return (u64)__builtin_amdgcn_ballot_w64(c); };

    // ---- the shared first term
    const u32 qt0 = row0 * T;
    const u32* hrow = p.bounds + (u64)qt0 * (p.n_tiles + 1) + tile;
    const u32 h0 = loose ? 0u : hrow[0], h1 = loose ? 0u : hrow[1];
    const sa_u64x2 hbs = ((const sa_u64x2*)p.qbase_imp)[qt0];
    const float hidf = p.idf[qt0];

    // ---- half tables of the queries' further terms: lane (qi, t) looks up term t's slice of query qi in this
    //      tile and writes one entry per 64 postings, in query-term order
    const u32 TT = gp.tt, tsh = gp.tt_shift, QPP = 64u >> tsh;
    // round 5: an item holds up to 64 queries of its group and takes them in PASSES of gp.cq (<= 16): the tables are built per
    // pass, the base -- and everything in front of it: block -> (tile, group), group entry, the shared term's slice and dense row --
    // once per item (cq0: first query of the pass, nq: its queries)
    u32 cq0 = 0u, nq = n < gp.cq ? n : gp.cq;
    struct Pre { u32 r0, r1; u64 base, send; float idf; };
    auto pre_load = [&](u32 ps) -> Pre {
        Pre x; x.r0 = 0; x.r1 = 0; x.base = 0; x.send = 0; x.idf = 0.f;
        const u32 qi = ps * QPP + (lane >> tsh), t = (loose ? 0u : 1u) + (lane & (TT - 1u));
        if (qi < nq && t < T) {
            const u32 qt = (row0 + cq0 + qi) * T + t;
            const u32* row = p.bounds + (u64)qt * (p.n_tiles + 1) + tile;
            const sa_u64x2 bs = ((const sa_u64x2*)p.qbase_imp)[qt];
            x.base = bs.x; x.send = bs.y;
            x.r0 = row[0]; x.r1 = row[1]; x.idf = p.idf[qt];
        }
        return x;
    };
    auto pre_store = [&](u32 ps, const Pre& x) {
        const u32 qi = ps * QPP + (lane >> tsh), tl = lane & (TT - 1u);
        const u32 np = x.r1 - x.r0;                             // postings of this term in this tile
        const u32 halves = (np + 63u) >> 6;
        u32 incl = halves;                                      // inclusive scan over the TT lanes of a query
        for (u32 o = 1; o < TT; o <<= 1) {
            const u32 up = __shfl_up(incl, o, SA_WAVE);
            if (tl >= o) incl += up;
        }
        const u32 excl = incl - halves;
        const u32 total = (u32)__shfl((int)incl, (int)(lane | (TT - 1u)), SA_WAVE);
        if (qi < nq) {
            s_idf[qi * TT + tl] = x.idf;
            const u64 c0 = x.base + x.r0;                       // first cell of the slice
            const u64 nhf = (u64)(total <= (u32)NH ? total : SA_GRPH_OVER) << SA_GRPH_NH_SHIFT;
            for (u32 j = 0; j < halves && excl + j < (u32)NH; j++) {
                const u64 c = c0 + (u64)j * 64ull;
                const u64 lim = (np - j * 64u < 64u ? np - j * 64u : 64u) - 1u;     // last posting of the half
                s_half[qi][excl + j] = (u64)(stream + c) | (lim << SA_GRPH_LIM_SHIFT) | ((u64)tl << SA_GRPH_TERM_SHIFT) |
                                       (excl + j == 0u ? nhf : 0ull);
            }
            // a query without postings: an entry 0 that says "0 halves"
            if (tl == 0u && total == 0u) s_half[qi][0] = (u64)(stream + p.imp_tail);
        }
    };
    // the shared term's dense factor row, requested BEFORE the tables are built (round 5: its latency used to start after them)
    float4 dv[TILE / 256];
    if (dslot != 0xFFFFFFFFu) {
        const float4* row4 = (const float4*)(gp.dense + (u64)dslot * gp.dense_stride + tile_base);
#pragma unroll
        for (int j = 0; j < TILE / 256; j++) dv[j] = row4[j * 64 + (int)lane];
    }
    SA_PTV(9);                                                  // (fine: group entry, first term's slice bounds, stream base, weight)
    auto build_tables = [&]() {
        const u32 NP = (nq + QPP - 1u) / QPP;                   // 1 or 2 lane passes (host: cq * TT <= 128)
        __builtin_amdgcn_wave_barrier();
        const Pre x0 = pre_load(0);
        Pre x1 = x0;
        if (NP > 1u) x1 = pre_load(1);
        SA_PTV(10);                                             // (fine: the further terms' slice bounds)
        pre_store(0, x0);
        if (NP > 1u) pre_store(1, x1);
        // One wave per workgroup: its LDS instructions execute in program order for all lanes, so lanes hand data
        // to each other through LDS without s_barrier; the wave barriers only pin the order of the accesses
        // for the compiler (they emit no instruction).
        __builtin_amdgcn_wave_barrier();
    };
    build_tables();
    if (n <= gp.cq) {
        // nothing to score in this tile at all?
        const u32 mine = lane < n ? (u32)(s_half[lane][0] >> SA_GRPH_NH_SHIFT) : 0u;
        if (h1 == h0 && ballot(mine != 0u) == 0ull) return;
    }
    SA_PT(0);                                                   // tables of the item built

    // The half descriptors of a query reach the scalar registers with ONE LDS instruction: lane h reads entry h
    // (8 bytes) and v_readlane hands the fields out -- no LDS round trip per half; a second one brings the query's
    // weights (lane t: term t).
    struct Q { u64 v[NH]; u32 dlo, dhi; float w; };
    typedef const __attribute__((address_space(1))) u64* gptr_u64;
    // request the postings of query qi's halves (dynamic number of loads: the caller has made sure that no
    // older load is outstanding, so "everything landed" is an exact wait for them later) and its bound
    auto prefetch = [&](u32 qi, Q& X) {
        const u64 d = s_half[qi][lane < (u32)NH ? lane : 0u];
        X.dlo = (u32)d; X.dhi = (u32)(d >> 32);
        X.w = s_idf[qi * TT + ((X.dhi >> (SA_GRPH_TERM_SHIFT - 32)) & 0x1Fu)];     // lane h: the weight of half h's term
        const u32 nh_raw = (u32)__builtin_amdgcn_readfirstlane((int)X.dhi) >> (SA_GRPH_NH_SHIFT - 32);
        // (too many: the pair goes to the per-query kernel; an odd count: the empty partner entry is loaded too --
        //  nothing masks a half's lanes, its postings must be the sentinel's)
        const u32 nh = nh_raw <= (u32)NH ? nh_raw : 0u;
        sa_static_while_below<0, NH, 1>(nh, [&](auto hc) {       // (a query has ~3 halves on average)
            constexpr int h = decltype(hc)::value;
            const u32 hi = (u32)__builtin_amdgcn_readlane((int)X.dhi, h);
            const u64 a = (u64)(u32)__builtin_amdgcn_readlane((int)X.dlo, h) | ((u64)(hi & 0xFFFFu) << 32);
            const u32 lim = (hi >> (SA_GRPH_LIM_SHIFT - 32)) & 0x3Fu;
            X.v[h] = ((gptr_u64)a)[lane < lim ? lane : lim];     // lanes past the end: copies of the last posting
        });
    };
    // the queries' bounds, one per lane, read once per item (a bound only ever rises: a stale one is valid)
    u32 thr_all = lane < n ? __hip_atomic_load(&p.gthr[row0 + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    if (p.seed && lane < n) { const u32 sd = p.seed[row0 + lane]; thr_all = sd > thr_all ? sd : thr_all; }
    Q A, B;
    prefetch(0, A);                                             // in flight while the base is built
    SA_PTV(11);                                                 // (fine: bounds + query 0's postings)

    // ---- base: clear, then the first term's slice scored once (write-only: 0 + s0 = s0)
    u32 base_max;
    if (dslot != 0xFFFFFFFFu) {
        // the shared term has a dense factor row: lane = doc, four docs per 16-byte load and LDS store, no unpacking and no
        // scatter (docs without the term hold 0.0 -> 0.0 * idf = +0.0, what the cleared accumulator holds)
        float4* a4 = (float4*)accu;
        u32 lmax = 0;
#pragma unroll
        for (int j = 0; j < TILE / 256; j++) {
            float4 w;
            w.x = __fmul_rn(dv[j].x, hidf); w.y = __fmul_rn(dv[j].y, hidf); w.z = __fmul_rn(dv[j].z, hidf); w.w = __fmul_rn(dv[j].w, hidf);
            a4[j * 64 + (int)lane] = w;
            const u32 m0 = __float_as_uint(w.x) > __float_as_uint(w.y) ? __float_as_uint(w.x) : __float_as_uint(w.y);
            const u32 m1 = __float_as_uint(w.z) > __float_as_uint(w.w) ? __float_as_uint(w.z) : __float_as_uint(w.w);
            const u32 m = m0 > m1 ? m0 : m1;
            lmax = m > lmax ? m : lmax;
        }
        __builtin_amdgcn_wave_barrier();
        at(spare) = 0u;
        __builtin_amdgcn_wave_barrier();
        base_max = sa_wave_max_u32(lmax);
    } else {
        float4* a4 = (float4*)accu;
#pragma unroll
        for (int j = 0; j < TILE / 256; j++) a4[j * 64 + (int)lane] = make_float4(0.f, 0.f, 0.f, 0.f);
        __builtin_amdgcn_wave_barrier();
        const u64 lo = hbs.x + h0, hi = hbs.x + h1, a0 = lo & ~1ull;
        const u32 npairs = hi > lo ? (u32)((hi - a0 + 1) >> 1) : 0u;
        const u32 jc = (u32)((hbs.y - a0) >> 1);
        const sa_u64x2* pairs = (const sa_u64x2*)(stream + a0);
        u32 lmax = 0;
        constexpr int PF = 4;
        sa_u64x2 cur[PF], nxt[PF];
        if (npairs) {
#pragma unroll
            for (int u = 0; u < PF; u++) { const u32 j = (u32)u * 64u + lane; cur[u] = pairs[j < jc ? j : jc]; }
        }
        for (u32 first = 0; first < npairs; first += (u32)PF * 64u) {
            const bool more = first + (u32)PF * 64u < npairs;
            if (more) {
#pragma unroll
                for (int u = 0; u < PF; u++) { const u32 j = first + (u32)(PF + u) * 64u + lane; nxt[u] = pairs[j < jc ? j : jc]; }
            }
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const u32 d0 = (u32)(cur[u].x >> 32) - tile_base_b, d1 = (u32)(cur[u].y >> 32) - tile_base_b;
                const bool in0 = d0 < (u32)TILE * 4u, in1 = d1 < (u32)TILE * 4u;
                const u32 w0 = __float_as_uint(__fmul_rn(__uint_as_float((u32)cur[u].x), hidf));
                const u32 w1 = __float_as_uint(__fmul_rn(__uint_as_float((u32)cur[u].y), hidf));
                at(in0 ? d0 : spare) = w0;
                at(in1 ? d1 : spare) = w1;
                const u32 m0 = in0 ? w0 : 0u, m1 = in1 ? w1 : 0u;
                lmax = m0 > lmax ? m0 : lmax;
                lmax = m1 > lmax ? m1 : lmax;
            }
            if (more) {
#pragma unroll
                for (int u = 0; u < PF; u++) cur[u] = nxt[u];
            }
        }
        __builtin_amdgcn_wave_barrier();
        at(spare) = 0u;                                         // (took the base's out-of-tile postings; the overlay's spare values start at 0)
        __builtin_amdgcn_wave_barrier();
        base_max = sa_wave_max_u32(lmax);
    }

    if constexpr (FILT) {
        if (!loose) {                                           // the base without the non-eligible docs (lane: four docs of one filter word per step)
            float4* a4 = (float4*)accu;
            u32 lmax = 0;
#pragma unroll
            for (int j = 0; j < TILE / 256; j++) {
                const u32 doc0 = (u32)(j * 64 + (int)lane) * 4u;
                const u64 fw = tile_base + doc0 < p.n_docs ? p.filt[(tile_base + doc0) >> 6] : 0ull;
                const u32 bits = (u32)(fw >> (doc0 & 63u)) & 15u;
                float4 v = a4[j * 64 + (int)lane];
                v.x = (bits & 1u) ? v.x : 0.f; v.y = (bits & 2u) ? v.y : 0.f; v.z = (bits & 4u) ? v.z : 0.f; v.w = (bits & 8u) ? v.w : 0.f;
                a4[j * 64 + (int)lane] = v;
                const u32 m0 = __float_as_uint(v.x) > __float_as_uint(v.y) ? __float_as_uint(v.x) : __float_as_uint(v.y);
                const u32 m1 = __float_as_uint(v.z) > __float_as_uint(v.w) ? __float_as_uint(v.z) : __float_as_uint(v.w);
                const u32 m = m0 > m1 ? m0 : m1;
                lmax = m > lmax ? m : lmax;
            }
            __builtin_amdgcn_wave_barrier();
            base_max = sa_wave_max_u32(lmax);
        }
    }
    SA_PT(1);                                                   // first query requested, base built
    // queries left to the per-query kernel (work list at the end)
    u64 deferred = 0ull;
    // survivors out: one reservation per query with survivors (lane qi reserves for query qi: the atomics travel
    // together), every buffered entry to its place (the buffer is in query order: an entry's offset inside its query
    // is its index minus the exclusive prefix of the per-query counts), bounds re-derived where a list crossed a
    // multiple of SA_GRP_REFRESH_STEP entries
    u32 nsurv = 0, my_surv = 0;                                  // buffered (wave-uniform); lane qi: those of query qi
    auto flush = [&]() {
        __builtin_amdgcn_wave_barrier();
        u32 cbase = 0;
        if (my_surv) cbase = atomicAdd(&p.cand_cnt[row0 + lane], my_surv);
        u32 start = my_surv;
#pragma unroll
        for (int o = 1; o < SA_WAVE; o <<= 1) {
            const u32 up = (u32)__shfl_up((int)start, (unsigned)o, SA_WAVE);
            if (lane >= (u32)o) start += up;
        }
        start -= my_surv;
        for (u32 e0 = 0; e0 < nsurv; e0 += (u32)SA_WAVE) {
            const u32 e = e0 + lane;
            const bool have = e < nsurv;
            const u64 ent = s_surv[have ? e : 0u];
            const u32 eq = (u32)ent & 0x3Fu, sl = (u32)ent >> 6, fin = (u32)(ent >> 32);
            const u32 qb = (u32)__shfl((int)cbase, (int)eq, SA_WAVE), qs = (u32)__shfl((int)start, (int)eq, SA_WAVE);
            if (have) {
                const u32 q = row0 + eq;
                atomicAdd(&p.hist[(u64)q * SA_HBINS + sa_score_bin(fin)], 1u);
                const u32 pos = qb + (e - qs);
                const u64 doc = p.doc_base + tile_base + (u64)(sl >> 2);
                if (pos < p.cand_cap) p.cand[(u64)q * p.cand_cap + pos] = ((u64)fin << 32) | (u64)(u32)(~(u32)doc);
            }
        }
        const bool crossed = my_surv != 0u && cbase / (u32)SA_GRP_REFRESH_STEP != (cbase + my_surv) / (u32)SA_GRP_REFRESH_STEP;
        for (u64 m = ballot(crossed); m; m &= m - 1ull) {
            const u32 q = row0 + (u32)__builtin_ctzll(m);
            sa_hist_refresh(p.hist + (u64)q * SA_HBINS, &p.gthr[q], p.k, lane);
        }
        __builtin_amdgcn_wave_barrier();
        nsurv = 0; my_surv = 0;
    };
    // One query of the item.  Per half, IN QUERY-TERM ORDER: read the docs' accumulators, add, write back with the sign
    // bit set ("touched by this query"; written as -(|o| + s), one instruction), remember what was read.  Nothing is
    // decided per lane: a lane outside the half's postings holds a copy of its last posting (an empty partner half:
    // the zero sentinel, which min(d, spare) sends to the lane's spare slot).  Then the base values go back -- every lane rewrites what it READ, the halves
    // in REVERSE order, so that for a doc touched by several terms the value read first (the base) is written last:
    // no lane needs to know whether it was the first to touch its doc.  The final scores are only looked at when the
    // largest value any lane wrote reaches the query's bound (one compare per query instead of a read, a mask and
    // two compares per half): then every doc's final value is read before the restore and the first touchers
    // (sign bit of what they read) report the docs that reach the bound.
    auto process = [&](u32 qi, const Q& X) {
        const u32 nh_raw = (u32)__builtin_amdgcn_readfirstlane((int)X.dhi) >> (SA_GRPH_NH_SHIFT - 32);
        const u32 gq = cq0 + qi;                                // the query's place in the item (its lane of thr_all / my_surv, its bit of deferred)
        const u32 thr_q = (u32)__builtin_amdgcn_readlane((int)thr_all, (int)gq);
        const u32 thr = thr_q > 1u ? thr_q : 1u;
        if (nh_raw > (u32)NH || base_max >= thr) { deferred |= 1ull << gq; return; }
        if (nh_raw == 0u) return;                               // the query scores exactly the base here: all below its bound
        const u32 nh = nh_raw;                                  // (round 4: an odd count no longer gets an empty partner half)
        u32 rs[NH], ro[NH];
        u32 wmax = 0u;                                          // largest value written (sign bit set)
        sa_static_while_below<0, NH, 1>(nh, [&](auto hc) {
            constexpr int h = decltype(hc)::value;
            {
                __builtin_amdgcn_wave_barrier();                // a half sees the previous half's (other lanes') writes
                const float w = __uint_as_float((u32)__builtin_amdgcn_readlane((int)__float_as_uint(X.w), h));
                const u64 v = X.v[h];
                const u32 d = (u32)(v >> 32) - tile_base_b;
                const u32 sl = d < spare ? d : spare;           // (a doc outside the tile: d >= TILE * 4)
                const u32 o = at(sl);
                __builtin_amdgcn_wave_barrier();                // (all lanes have read -- copies of a posting read the same value -- before any writes)
                const u32 nw = __float_as_uint(__fsub_rn(-fabsf(__uint_as_float(o)), __fmul_rn(__uint_as_float((u32)v), w)));
                at(sl) = nw;
                wmax = nw > wmax ? nw : wmax;
                rs[h] = sl;
                ro[h] = o;
            }
        });
        __builtin_amdgcn_wave_barrier();
        const bool look = ballot(wmax >= (thr | 0x80000000u)) != 0ull;
        u32 fin[NH];
        if (look) {                                             // (rare once the bound stands)
#pragma unroll
            for (int h = 0; h < NH; h++) fin[h] = (u32)h < nh ? at(rs[h]) & 0x7FFFFFFFu : 0u;
            __builtin_amdgcn_wave_barrier();
        }
        // base values back, last half first
        auto back = [&](auto hc) {
            constexpr int h = decltype(hc)::value;
            at(rs[h]) = ro[h];
            __builtin_amdgcn_wave_barrier();
        };
        // (nh = 1 .. NH; the usual 2 or 3 halves cost three or four scalar tests -- as a switch with fall-through the compiler
        //  built a chain of ~25 scalar flag operations in front of the stores of the usual case)
        static_assert(NH == 10, "restore chain");
        if (nh > 4u) {
            if (nh > 8u) { if (nh > 9u) back(std::integral_constant<int, 9>{}); back(std::integral_constant<int, 8>{}); }
            if (nh > 6u) { if (nh > 7u) back(std::integral_constant<int, 7>{}); back(std::integral_constant<int, 6>{}); }
            if (nh > 5u) back(std::integral_constant<int, 5>{});
            back(std::integral_constant<int, 4>{});
        }
        if (nh > 2u) { if (nh > 3u) back(std::integral_constant<int, 3>{}); back(std::integral_constant<int, 2>{}); }
        if (nh > 1u) back(std::integral_constant<int, 1>{});
        back(std::integral_constant<int, 0>{});
        if (!look) return;
        u64 kb[NH];
        u32 c = 0;
#pragma unroll
        for (int i = 0; i < NH; i++) {
            kb[i] = 0ull;
            if ((u32)i < nh) {
                const u32 lim = ((u32)__builtin_amdgcn_readlane((int)X.dhi, i) >> (SA_GRPH_LIM_SHIFT - 32)) & 0x3Fu;
                bool el = true;
                if constexpr (FILT) {                           // the doc's filter bit (this path is rare once the bound stands)
                    const u32 dd = rs[i] >> 2;
                    const bool inr = rs[i] < (u32)TILE * 4u && tile_base + dd < p.n_docs;
                    const u64 fw = p.filt[inr ? (tile_base + dd) >> 6 : 0ull];
                    el = inr && ((fw >> (dd & 63u)) & 1ull) != 0ull;
                }
                kb[i] = ballot(lane <= lim && rs[i] < (u32)TILE * 4u && !(ro[i] >> 31) && fin[i] >= thr && el);
            }
            c += (u32)__popcll(kb[i]);
        }
        if (c == 0u) return;
        if (c > 16u) { deferred |= 1ull << gq; return; }        // bound still far off: the per-query item's histogram path refines it first
        // Survivors are buffered in LDS and written out together (flush below): reserving places in a query's
        // candidate list is an atomic WITH a return value -- a round trip to L2 the wave sits out; per surviving pair
        // that was most of the 0.45 ms the candidates cost at k = 1000.  Flushed, the reservations of all queries of
        // the item travel together.
        if (nsurv + c > (u32)SA_GRP_SURV_CAP) flush();
        const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
        for (int i = 0; i < NH; i++) {
            if (kb[i]) {                                        // (uniform: halves without survivors cost a scalar test)
                if ((kb[i] >> lane) & 1ull) s_surv[nsurv + (u32)__popcll(kb[i] & lt)] = ((u64)fin[i] << 32) | (u64)(rs[i] << 6) | (u64)gq;
                nsurv += (u32)__popcll(kb[i]);
            }
        }
        if (lane == gq) my_surv = c;
    };

    // ---- the queries of the group, two per round so that the prefetch buffers swap without copies.  Before the
    //      next query's loads are issued everything older has landed (an exact wait: only the current query's
    //      loads are outstanding), so the current query is processed while exactly the next one's loads fly.
    for (;;) {
        for (u32 qi = 0; qi < nq; qi += 2) {
            SA_WAIT_VMCNT0();
            SA_PT(2);
            if (qi + 1u < nq) prefetch(qi + 1u, B);
            SA_PT(3);
            process(qi, A);
            SA_PT(4);
            if (qi + 1u < nq) {
                SA_WAIT_VMCNT0();
                SA_PT(2);
                if (qi + 2u < nq) prefetch(qi + 2u, A);
                SA_PT(3);
                process(qi + 1u, B);
                SA_PT(4);
            }
        }
        // the item's next pass: tables of its next queries over the same base
        cq0 += nq;
        if (cq0 >= n) break;
        nq = n - cq0 < gp.cq ? n - cq0 : gp.cq;
        build_tables();
        prefetch(0, A);
        SA_PT(0);
    }
    if (nsurv) flush();
    // ---- general path: hand the (tile, query) pairs to the per-query kernel that follows (sa_k_bm25_tiles_wl)
    if (deferred) {
        const u32 c = (u32)__popcll(deferred);
        u32 wbase = 0;
        if (lane == 0) wbase = atomicAdd(gp.wl_cnt, c);
        wbase = (u32)__builtin_amdgcn_readfirstlane((int)wbase);
        if ((deferred >> lane) & 1ull)
            gp.wl[wbase + (u32)__popcll(deferred & ((1ull << lane) - 1ull))] = ((u64)tile << 32) | (u64)(row0 + lane);
    }
#ifdef SA_PROBE
    SA_PT(5);
    if (lane == 0) {
        unsigned long long* const ps = g_sa_probe + (size_t)(blockIdx.x % SA_PROBE_SLOTS) * 16;
        for (int i = 0; i < 6; i++) atomicAdd(&ps[i], pacc[i]);
        for (int i = 9; i < 12; i++) atomicAdd(&ps[i], pacc[i]);
        atomicAdd(&ps[6], 1ull);
        atomicAdd(&ps[7], (unsigned long long)n);
        atomicAdd(&ps[8], (unsigned long long)__popcll(deferred));
    }
#endif
}

// The (tile, query) items the grouped kernel left to the per-query path (usually none once the bounds stand):
// their number is only known on the device, so a resident grid walks the work list.
template <int TILE, int THREADS>
__global__ void __launch_bounds__(THREADS) sa_k_bm25_tiles_wl(const Bm25Params p, const u64* __restrict__ wl,
                                                               const u32* __restrict__ wl_cnt) {
    __shared__ alignas(16) u64 smem[sa_tile_smem_u64<TILE, 1>()];
    __shared__ float s_tab[sa_tile_tab_floats<THREADS, true>()];
    const u32 nitems = *wl_cnt;
    for (u32 i = blockIdx.x; i < nitems; i += gridDim.x) {
        const u64 it = wl[i];
        sa_bm25_tile_item<TILE, THREADS, 1, true>(p, (u32)(it >> 32), (u32)it, smem, s_tab);
        __syncthreads();                              // LDS is reused by the next item
    }
}

// Merge n_cand candidate keys per query into the k best, sorted descending.
// One workgroup of 1024 threads per query.
//
// Small rows (<= SA_MERGE_LIST keys: a cross-rank merge, or a well-pruned append list) go straight
// into LDS and a bitonic sort finishes.  Larger rows are first cut by a lower bound of the k-th
// largest key that is already known:
//   gthr / slots       the bound the tile kernel left behind (>= k docs score at or above it)
//   rank_stride > 0    rows made of sorted groups of rank_stride keys: the k-th largest GROUP
//                      LEADER bounds the k-th largest key (k distinct groups own a key >= it)
// One pass keeps the keys above the bound in LDS.  If they overflow the LDS list (large k, ties)
// the survivors are compacted in place at the front of the row and the exact k-th largest is
// found by MSB-first bisection over the survivors only.

// clears `words` u32 at `slots` and `n8` 8-byte cells at `bloom`
__global__ void __launch_bounds__(256)
sa_k_run_reset(u32* __restrict__ slots, u64 words, u64* __restrict__ bloom, u64 n8, u32* __restrict__ one_more) {
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0 && one_more) *one_more = 0u;
    for (u64 i = t; i < words; i += stride) slots[i] = 0u;
    for (u64 i = t; i < n8; i += stride) bloom[i] = 0ull;
}

// (THREADS: 1024, or 256 for small k -- a workgroup of 16 waves needs 16 free wave slots and 17 KiB of LDS on ONE CU at once, which a
//  device full of one-wave scoring workgroups hands out slowly; for k <= 64 a query has a few dozen candidates and four waves do)
template <int THREADS>
__global__ void __launch_bounds__(THREADS)
sa_k_topk_merge(u64* __restrict__ cand, u32 n_cand_max, u32 k, u64* __restrict__ out,
                const u32* __restrict__ out_row, u32 rank_stride, const u32* __restrict__ cnt,
                const u32* __restrict__ slots, const u32* __restrict__ gthr, u32* __restrict__ overflow,
                u32* __restrict__ clr_state, u32 clr_B, u32 clr_hist, u32* __restrict__ clr_one,
                u32 gather_stride, u32* __restrict__ xflag, const u32* __restrict__ seed) {
    constexpr int NW = THREADS / SA_WAVE;
    __shared__ u64 red64[NW + 1];
    __shared__ u64 sel[SA_MERGE_LIST];
    __shared__ u32 s_n;
    const u32 q = blockIdx.x, tid = threadIdx.x;
    if (gather_stride) {
        // The row is read straight out of an all-gather result [rank][B*k + 1] (no regroup launch): key i of query q is
        // key i % k of rank i / k; the extra cell of every rank's block is its overflow flag, OR-ed into *xflag.
        // Only rows that fit the LDS list take this route (the host checks), so nothing is compacted in place.
        if (tid == 0) s_n = 0;
        for (u32 i = tid; i < SA_MERGE_LIST; i += THREADS) sel[i] = 0;
        __syncthreads();
        const u32 B_ = gridDim.x;
        for (u32 i = tid; i < n_cand_max; i += THREADS) {
            const u32 r = i / rank_stride, j = i % rank_stride;
            const u64 x = cand[(u64)r * gather_stride + (u64)q * rank_stride + j];
            if (x) { const u32 pos = atomicAdd(&s_n, 1u); sel[pos] = x; }
        }
        if (q == 0 && tid == 0 && xflag) {
            u32 any = 0;
            for (u32 r = 0; r < n_cand_max / rank_stride; r++) any |= cand[(u64)r * gather_stride + (u64)B_ * rank_stride] != 0ull ? 1u : 0u;
            if (any) *xflag = 1u;
        }
        __syncthreads();
        const u32 n_sel = s_n;
        u32 np2 = 2;
        while (np2 < n_sel) np2 <<= 1;
        sa_block_bitonic_desc(sel, np2);
        const u32 row_ = out_row ? out_row[q] : q;
        for (u32 i = tid; i < k; i += THREADS) out[(u64)row_ * k + i] = (i < SA_MERGE_LIST) ? sel[i] : 0ull;
        return;
    }
    u64* c = cand + (u64)q * n_cand_max;
    // cnt != null: the row is an append list holding cnt[q] keys (pruned tile selection)
    u32 n_cand = n_cand_max;
    if (cnt) {
        const u32 have = cnt[q];
        n_cand = have < n_cand_max ? have : n_cand_max;
        if (have > n_cand_max && overflow && tid == 0) atomicMax(overflow, 1u);   // the list ran over: see sa_batch_fetch
    }
    const u32 row = out_row ? out_row[q] : q;       // device row q holds caller query out_row[q]
    for (u32 i = tid; i < SA_MERGE_LIST; i += THREADS) sel[i] = 0;
    if (tid == 0) s_n = 0;
    __syncthreads();

    // MSB-first bisection (2 bits per step) for the k-th largest of c[0 : n : stride]
    auto kth_largest = [&](u32 n, u32 stride) -> u64 {
        u64 m = 0;
        for (u32 i = tid; i < n; i += THREADS) { const u64 x = c[(u64)i * stride]; m = x > m ? x : m; }
        m = sa_block_max64<NW>(m, red64);
        if (m == 0 || n < k) return 0;
        int top = 63 - __clzll((long long)m);
        if ((top & 1) == 0) top++;
        u64 prefix = 0;
        for (int bit = top; bit >= 1; bit -= 2) {
            const u64 c1 = prefix | (1ull << (bit - 1)), c2 = prefix | (2ull << (bit - 1)), c3 = prefix | (3ull << (bit - 1));
            u64 packed = 0;
            for (u32 i = tid; i < n; i += THREADS) {
                const u64 x = c[(u64)i * stride];
                packed += (x >= c1 ? 1ull : 0ull) + (x >= c2 ? (1ull << 21) : 0ull) + (x >= c3 ? (1ull << 42) : 0ull);
            }
#pragma unroll
            for (int o = SA_WAVE / 2; o > 0; o >>= 1) packed += __shfl_xor(packed, o, SA_WAVE);
            if (sa_lane() == 0) red64[sa_wave_id()] = packed;
            __syncthreads();
            u64 tot = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) tot += red64[w];
            __syncthreads();
            const u32 n1 = (u32)(tot & 0x1FFFFF), n2 = (u32)((tot >> 21) & 0x1FFFFF), n3 = (u32)((tot >> 42) & 0x1FFFFF);
            if (n3 >= k) prefix = c3; else if (n2 >= k) prefix = c2; else if (n1 >= k) prefix = c1;
        }
        return prefix;
    };

    u64 thr = 1;
    if (gthr) {
        // histogram bound left behind by the scoring kernels: at least k docs score >= it, so only
        // keys at or above it matter -- usually a few dozen, sorted by one wave below
        thr = (u64)gthr[q] << 32;
        if (thr < 1) thr = 1;
    } else if (n_cand > SA_MERGE_LIST) {
        if (slots) {
            u32 g = slots[(u64)q * 32 + (tid & 31)];
            g = sa_wave_min_u32(g);                   // every wave computes the same minimum
            thr = (u64)g << 32;
        } else if (rank_stride > 0 && n_cand / rank_stride >= k) {
            thr = kth_largest(n_cand / rank_stride, rank_stride);
        }
        if (thr < 1) thr = 1;
    }
    for (u32 i = tid; i < n_cand; i += THREADS) {
        const u64 x = c[i];
        if (x >= thr) {
            const u32 pos = atomicAdd(&s_n, 1u);
            if (pos < SA_MERGE_LIST) sel[pos] = x;
        }
    }
    __syncthreads();
    u32 n_sel = s_n;
    __syncthreads();
    if (n_sel > SA_MERGE_LIST) {                      // uniform
        // compact the survivors to the front of the row (a chunk's writes land below its own
        // end: at most as many survivors as keys read so far), then bisect over them only
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (u32 base = 0; base < n_cand; base += 4 * THREADS) {
            u64 x[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const u32 i = base + j * THREADS + tid;
                x[j] = i < n_cand ? c[i] : 0ull;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (x[j] >= thr) c[atomicAdd(&s_n, 1u)] = x[j];
        }
        __syncthreads();
        const u32 n_surv = s_n;
        __syncthreads();
        const u64 g = kth_largest(n_surv, 1);         // exact: keys are distinct, so exactly k keys are >= g
        thr = g > 1 ? g : 1;
        for (u32 i = tid; i < SA_MERGE_LIST; i += THREADS) sel[i] = 0;
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (u32 i = tid; i < n_surv; i += THREADS) {
            const u64 x = c[i];
            if (x >= thr) {
                const u32 pos = atomicAdd(&s_n, 1u);
                if (pos < SA_MERGE_LIST) sel[pos] = x;
            }
        }
        __syncthreads();
        n_sel = s_n;
    }
    // Fewer than k keys at or above a bound: with bounds derived from k counted docs, or from a term's k-th largest factor,
    // that cannot happen -- a safety net under the starting bounds (a rank table out of step with the impact stream, a
    // scoring path whose rounding broke the monotonicity argument): the run is flagged and redone without bounds.
    if (gthr && overflow && n_sel < k && tid == 0 && (gthr[q] != 0u || (seed && seed[q] != 0u))) atomicMax(overflow, 2u);
    n_sel = n_sel < SA_MERGE_LIST ? n_sel : SA_MERGE_LIST;
    if (n_sel <= SA_WAVE) {                           // uniform
        // short list: one wave sorts it in registers (bitonic over lanes, no barriers)
        if (tid < SA_WAVE) {
            u64 x = sel[tid];                         // slots past n_sel are 0
#pragma unroll
            for (u32 size = 2; size <= SA_WAVE; size <<= 1) {
#pragma unroll
                for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
                    const u64 y = __shfl_xor(x, (int)stride, SA_WAVE);
                    const bool lower = (tid & stride) == 0;           // this lane holds the pair's lower index
                    const bool desc = (tid & size) == 0;
                    const bool take_max = lower == desc;
                    x = take_max ? (x > y ? x : y) : (x < y ? x : y);
                }
            }
            sel[tid] = x;
        }
        __syncthreads();
    } else {
        u32 np2 = 2;
        while (np2 < n_sel) np2 <<= 1;
        sa_block_bitonic_desc(sel, np2);
    }
    for (u32 i = tid; i < k; i += THREADS) out[(u64)row * k + i] = (i < SA_MERGE_LIST) ? sel[i] : 0ull;
    // The merge is the last reader of the run's per-query state, so it leaves it zeroed for the next run of the
    // batch -- bound slots [B][32], cursors [B], cached bounds [B], histograms [B][SA_HBINS] (layout: sa_batch_alloc_topk),
    // the grouped kernel's work-list cursor -- instead of a reset launch in front of every run.
    if (clr_state) {
        if (tid < 32u) clr_state[(u64)q * 32u + tid] = 0u;
        if (tid == 32u) clr_state[(u64)clr_B * 32u + q] = 0u;
        if (tid == 33u) clr_state[(u64)clr_B * 33u + q] = 0u;
        if (clr_hist) for (u32 i = tid; i < (u32)SA_HBINS; i += THREADS) clr_state[(u64)clr_B * 34u + (u64)q * SA_HBINS + i] = 0u;
        if (clr_one && q == 0u && tid == 34u) *clr_one = 0u;
    }
}


// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------

void sa_launch_run_reset(u32* slots, u64 words, u64* bloom, u64 n8, u32* one_more, hipStream_t st) {
    const u64 work = words + n8 + 1;
    const u32 grid = work / 256 + 1 < 2048 ? (u32)(work / 256 + 1) : 2048u;
    hipLaunchKernelGGL(sa_k_run_reset, dim3(grid), dim3(256), 0, st, slots, words, bloom, n8, one_more);
}

void sa_fill_params(const sa_index* ix, Bm25Params& p) {
    p.tfp = ix->d_tfp; p.tf_off = ix->d_tf_off; p.dir_slot = ix->d_dir_slot; p.tile_dir = ix->d_tile_dir;
    p.doc_lens = ix->d_doc_lens; p.n_terms = ix->n_terms; p.n_tiles = ix->n_tiles;
    p.n_docs = ix->n_docs; p.doc_base = ix->doc_base; p.dl_packed = ix->dl_packed ? 1 : 0;
    p.avgdl = ix->avg_doc_len;
    p.qlist = nullptr; p.nq = 0;                     // callers set nq (= B) after filling B
    p.tile0 = 0; p.tile_end = ix->n_tiles;
}

u32 sa_tile_waves(u32 tile_docs) {
    switch (tile_docs) {
        case 1024: return 2; case 2048: return 1; case 4096: return 2; case 8192: return 4;
        case 16384: return 8; case 32768: return 16; default: return 1;
    }
}

int sa_launch_make_sattab(sa_index* ix, float* d_tab, u32* tab_w_out, float k1, float b, hipStream_t st) {
    u32 w = 0;
    if (ix->dl_packed) {
        w = 64;
        while (w < SA_SAT_WMAX && w <= ix->max_doc_len) w <<= 1;
    }
    *tab_w_out = w;
    if (w) hipLaunchKernelGGL(sa_k_make_sattab, dim3(sa_div_up((u64)SA_SAT_NTF * w, 256)), dim3(256), 0, st, d_tab, w, k1, b,
                              ix->avg_doc_len);
    return SA_OK;
}

int sa_launch_make_bounds(sa_index* ix, const u32* d_terms, u32 BT, u32* d_bounds, u64* d_qbase, hipStream_t st, u64* d_qbase_imp,
                          const float* d_topf, const float* d_idf, u32 T, u32 k, u32* d_seed, float seed_scale) {
    const u64 total = (u64)BT * (ix->n_tiles + 1);
    if (total == 0) return SA_OK;
    const u32 grid = total / 256 + 1 < 8192 ? (u32)(total / 256 + 1) : 8192;
    u32 rank_idx = SA_TOPF_NR - 1;                               // the smallest tabulated rank >= k
    for (int i = SA_TOPF_NR - 1; i >= 0; i--) if (sa_topf_ranks[i] >= k) rank_idx = (u32)i;
    hipLaunchKernelGGL(sa_k_make_bounds, dim3(grid), dim3(256), 0, st, ix->d_tfp, ix->d_tf_off, ix->d_dir_slot,
                       ix->d_tile_dir, ix->n_terms, ix->n_tiles, ix->tile_docs, d_terms, BT, d_bounds, d_qbase, d_qbase_imp,
                       d_topf, d_idf, T, rank_idx, (d_topf && d_idf) ? d_seed : (u32*)nullptr, seed_scale);
    return SA_OK;
}


#define SA_LAUNCH_TILE_MM(TILE, THREADS)                                                           \
    {                                                                                              \
        if (MODE == 1 && p.imp && p.occur_off)                                                     \
            hipLaunchKernelGGL((sa_k_bm25_tiles<TILE, THREADS, MODE, MODE == 1, 2>), grid, dim3(THREADS), 0, st, p); \
        else if (p.occur_off)                                                                      \
            hipLaunchKernelGGL((sa_k_bm25_tiles<TILE, THREADS, MODE, false, 2>), grid, dim3(THREADS), 0, st, p); \
        else if (MODE == 1 && p.imp)                                                               \
            hipLaunchKernelGGL((sa_k_bm25_tiles<TILE, THREADS, MODE, MODE == 1, 1>), grid, dim3(THREADS), 0, st, p); \
        else                                                                                       \
            hipLaunchKernelGGL((sa_k_bm25_tiles<TILE, THREADS, MODE, false, 1>), grid, dim3(THREADS), 0, st, p); \
    }                                                                                              \
    break

#define SA_LAUNCH_TILE(TILE, THREADS)                                                              \
    {                                                                                              \
        if (MODE == 1 && p.imp)                                                                    \
            hipLaunchKernelGGL((sa_k_bm25_tiles<TILE, THREADS, MODE, MODE == 1>), grid, dim3(THREADS), 0, st, p); \
        else                                                                                       \
            hipLaunchKernelGGL((sa_k_bm25_tiles<TILE, THREADS, MODE, false>), grid, dim3(THREADS), 0, st, p); \
    }                                                                                              \
    break

template <int MODE>
static int sa_launch_bm25_mode(sa_index* ix, const Bm25Params& p, hipStream_t st) {
    const u32 nt = p.tile_end - p.tile0;
    const u32 gy = nt < SA_GRID_Y ? nt : SA_GRID_Y;
    const dim3 grid(p.nq, gy, (nt + SA_GRID_Y - 1) / SA_GRID_Y);
    if (p.min_match_off) {                                      // the counting instantiations (sa_min_match_tiles; p.occur_off: those with occur classes)
        switch (ix->tile_docs) {
            case 1024: SA_LAUNCH_TILE_MM(1024, 128);
            case 2048: SA_LAUNCH_TILE_MM(2048, 64);
            case 4096: SA_LAUNCH_TILE_MM(4096, 128);
            case 8192: SA_LAUNCH_TILE_MM(8192, 256);
            default:
                sa_set_error("minimum-should-match / occur: no counting kernel for tile_docs %u", ix->tile_docs);
                return SA_ERR_UNSUPPORTED;
        }
        return SA_OK;
    }
    switch (ix->tile_docs) {
        case 1024: SA_LAUNCH_TILE(1024, 128);
        case 2048: SA_LAUNCH_TILE(2048, 64);
        case 4096: SA_LAUNCH_TILE(4096, 128);
        case 8192: SA_LAUNCH_TILE(8192, 256);
        case 16384: SA_LAUNCH_TILE(16384, 512);
        case 32768: SA_LAUNCH_TILE(32768, 1024);
        default:
            sa_set_error("unsupported tile_docs %u", ix->tile_docs);
            return SA_ERR_STATE;
    }
    return SA_OK;
}

#define SA_LAUNCH_LIST(TILE, THREADS)                                                              \
    {                                                                                              \
        if (p.imp)                                                                                 \
            hipLaunchKernelGGL((sa_k_bm25_tiles_list<TILE, THREADS, true>), dim3(grid), dim3(THREADS), 0, st, p); \
        else                                                                                       \
            hipLaunchKernelGGL((sa_k_bm25_tiles_list<TILE, THREADS, false>), dim3(grid), dim3(THREADS), 0, st, p); \
    }                                                                                              \
    break

// the tile sizes the counting (minimum-should-match) instantiations of the per-query tile kernel exist for
bool sa_min_match_tiles(u32 tile_docs) { return tile_docs == 1024 || tile_docs == 2048 || tile_docs == 4096 || tile_docs == 8192; }

int sa_launch_bm25_list(sa_index* ix, const Bm25Params& p, hipStream_t st) {
    if (ix->n_tiles == 0 || p.B == 0) return SA_OK;
    const u64 worst = (u64)p.B * ix->n_tiles;
    const u32 grid = worst < 4096 ? (u32)worst : 4096u;
    switch (ix->tile_docs) {
        case 1024: SA_LAUNCH_LIST(1024, 128);
        case 2048: SA_LAUNCH_LIST(2048, 64);
        case 4096: SA_LAUNCH_LIST(4096, 128);
        case 8192: SA_LAUNCH_LIST(8192, 256);
        default:
            sa_set_error("unsupported tile_docs %u for the query-list scan", ix->tile_docs);
            return SA_ERR_STATE;
    }
    return SA_OK;
}

// the facet pass over p's tiles and rows: the grid of sa_launch_bm25_mode, the MM the batch's counting state asks for.
// Workgroup sizes: TWICE those of sa_k_bm25_tiles for the same tile (16 documents per thread, 4 at 1024), on purpose -- an
// instantiation of the tile item that an existing kernel uses too would share the item's function-local LDS variables with it, and
// the compiler then allocates that kernel's registers differently (measured: the MODE 0 instantiations of 2048 docs and up came out
// with other VGPR counts).  With sizes of its own the pre-existing kernels' gfx950 code is what it was, instruction for instruction.
int sa_launch_bm25_facet(sa_index* ix, const Bm25Params& p, const FacetParams& fp, hipStream_t st) {
    if (ix->n_tiles == 0 || p.nq == 0 || p.tile_end <= p.tile0) return SA_OK;
    const u32 nt = p.tile_end - p.tile0;
    const u32 gy = nt < SA_GRID_Y ? nt : SA_GRID_Y;
    const dim3 grid(p.nq, gy, (nt + SA_GRID_Y - 1) / SA_GRID_Y);
#define SA_LAUNCH_FACET(TILE, THREADS)                                                                                            \
    {                                                                                                                             \
        if (p.occur_off) hipLaunchKernelGGL((sa_k_bm25_facet_tiles<TILE, THREADS, 2>), grid, dim3(THREADS), 0, st, p, fp);         \
        else if (p.min_match_off) hipLaunchKernelGGL((sa_k_bm25_facet_tiles<TILE, THREADS, 1>), grid, dim3(THREADS), 0, st, p, fp); \
        else hipLaunchKernelGGL((sa_k_bm25_facet_tiles<TILE, THREADS, 0>), grid, dim3(THREADS), 0, st, p, fp);                     \
    }                                                                                                                             \
    break
    switch (ix->tile_docs) {
        case 1024: SA_LAUNCH_FACET(1024, 256);
        case 2048: SA_LAUNCH_FACET(2048, 128);
        case 4096: SA_LAUNCH_FACET(4096, 256);
        case 8192: SA_LAUNCH_FACET(8192, 512);
        default:
            sa_set_error("facet counts: no counting kernel for tile_docs %u (1024, 2048, 4096, 8192)", ix->tile_docs);
            return SA_ERR_UNSUPPORTED;
    }
#undef SA_LAUNCH_FACET
    return SA_OK;
}

int sa_launch_bm25_groups(sa_index* ix, const sa_batch* bt, const Bm25Params& p, u32 tile0, hipStream_t st) {
    GroupParams gp;
    gp.grp = bt->d_grp; gp.n_groups = bt->n_groups;
    gp.tile0 = tile0; gp.n_tiles_run = ix->n_tiles - tile0;
    gp.tt = bt->grp_tt; gp.tt_shift = bt->grp_tt_shift; gp.cq = bt->grp_cq;
    gp.dense = (bt->impacts && sa_opt(bt->opts.group_dense, 1) != 0) ? bt->impacts->d_dense : nullptr;
    gp.dense_stride = bt->impacts ? bt->impacts->dense_stride : 0;
    const u64 blocks = (u64)((gp.n_tiles_run + 7u) / 8u) * 8u * gp.n_groups;
    gp.tpx = sa_opt(bt->opts.xcd_range, 1) != 0 ? (gp.n_tiles_run + 7u) / 8u : 0u;
    if (blocks > 0x7FFFFFFFull) { sa_set_error("grouped launch: bad grid"); return SA_ERR_STATE; }
    gp.wl = bt->d_wl; gp.wl_cnt = bt->d_wl_cnt;
    const u64 worst = (u64)gp.n_tiles_run * bt->n_grouped_rows;
    const u32 wgrid = worst < 2048 ? (u32)worst : 2048u;
    if (wgrid == 0) return SA_OK;
    // (weight table: n * tt cells; 64 cover up to 4 overlaid terms per query at 16 queries per item)
    const bool small = (u32)SA_GRP_MAXQ * gp.tt <= 64u;
#ifdef SA_PROBE
    // (measurement build: unused dynamic LDS per workgroup lowers the resident waves per CU -- the occupancy experiment of DESIGN 3.1a)
    const u32 lds_pad = getenv("SA_PROBE_LDS_PAD") ? (u32)atoi(getenv("SA_PROBE_LDS_PAD")) : 0u;
#else
    const u32 lds_pad = 0u;
#endif
#define SA_LAUNCH_GROUP(TILE, THREADS, FILT)                                                                               \
    {                                                                                                                      \
        if (blocks && small && p.filt) hipLaunchKernelGGL((sa_k_bm25_group_tiles<TILE, 64, (FILT)>), dim3((u32)blocks), dim3(64), lds_pad, st, p, gp);   \
        else if (blocks && p.filt) hipLaunchKernelGGL((sa_k_bm25_group_tiles<TILE, 128, (FILT)>), dim3((u32)blocks), dim3(64), lds_pad, st, p, gp);      \
        else if (blocks && small) hipLaunchKernelGGL((sa_k_bm25_group_tiles<TILE, 64, false>), dim3((u32)blocks), dim3(64), lds_pad, st, p, gp);       \
        else if (blocks) hipLaunchKernelGGL((sa_k_bm25_group_tiles<TILE, 128, false>), dim3((u32)blocks), dim3(64), lds_pad, st, p, gp);               \
        hipLaunchKernelGGL((sa_k_bm25_tiles_wl<TILE, THREADS>), dim3(wgrid), dim3(THREADS), 0, st, p, (const u64*)gp.wl,   \
                           (const u32*)gp.wl_cnt);                                                                         \
    }                                                                                                                      \
    break
    switch (ix->tile_docs) {
        case 1024: SA_LAUNCH_GROUP(1024, 128, true);
        case 2048: SA_LAUNCH_GROUP(2048, 64, true);
        // (4096-doc tiles: no filtered instantiation -- the kernel already misses its occupancy target there; the route rule keeps
        //  filtered batches of such an index on the per-query kernel, sa_batch_plan)
        case 4096:
            if (p.filt) { sa_set_error("grouped kernel: no filtered instantiation for 4096-doc tiles"); return SA_ERR_STATE; }
            SA_LAUNCH_GROUP(4096, 128, false);
        default:
            sa_set_error("unsupported tile_docs %u for the grouped kernel", ix->tile_docs);
            return SA_ERR_STATE;
    }
#undef SA_LAUNCH_GROUP
    return SA_OK;
}

int sa_launch_bm25(sa_index* ix, const Bm25Params& p, hipStream_t st) {
    if (ix->n_tiles == 0 || p.nq == 0 || p.tile_end <= p.tile0) return SA_OK;
    return p.pruned ? sa_launch_bm25_mode<1>(ix, p, st) : sa_launch_bm25_mode<0>(ix, p, st);
}


// ---- BASELINE config 2 as one launch (reference postings.py:652-680 score(), bm25.pyx:11-25; summed over the query terms as
// test/test_msmarco.py:353-354 does): the dense float32[n_docs] BM25 vector of T terms, written ONCE -- straight into the caller's
// device vector (times its boost) or into the scratch vector the host copy starts from.  A workgroup owns a tile of docs: zeroes
// its accumulators in LDS, adds factor x idf for every posting of every term in the tile (term after term, so a doc's sum is formed
// in query-term order exactly like the tile kernel's), stores the tile.  Bytes per call: 8 x (postings of the terms) + 4 x n_docs.
// The terms and weights travel in the kernel arguments: no upload, no slice-table launch (a slice's ends come from the index's own
// tile directory, or a search of the term's postings), no fill, no scale / copy pass.
struct DenseQuery { u32 term[SA_MAX_QTERMS]; float w[SA_MAX_QTERMS]; };

template <int TILE>
__global__ void __launch_bounds__(256)
sa_k_bm25_dense_direct(const u64* __restrict__ tfp, const u64* __restrict__ tf_off, const u32* __restrict__ dir_slot,
                       const u32* __restrict__ tile_dir, const u64* __restrict__ imp, u32 n_terms, u32 n_tiles, u64 n_docs,
                       const DenseQuery q, u32 T, float boost, int has_boost, float* __restrict__ out) {
    __shared__ alignas(16) float acc[TILE];
    __shared__ u64 s_first[SA_MAX_QTERMS];
    __shared__ u32 s_cnt[SA_MAX_QTERMS];
    const u32 tile = blockIdx.x, tid = threadIdx.x;
    const u64 d0 = (u64)tile * TILE;
    for (u32 i = tid; i < (u32)TILE / 4u; i += 256u) ((float4*)acc)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < T) {
        const u32 term = q.term[tid];
        u64 first = 0; u32 cnt = 0;
        if (term < n_terms) {
            const u64 base = tf_off[term];
            const u32 df = (u32)(tf_off[term + 1] - base);
            const u32 slot = dir_slot[term];
            u32 lo, hi;
            if (slot != 0xFFFFFFFFu) {
                lo = tile_dir[(u64)slot * (n_tiles + 1) + tile];
                hi = tile_dir[(u64)slot * (n_tiles + 1) + tile + 1u];
            } else {
                lo = sa_lower_bound(tfp + base, 0, df, d0 << SA_KEY_SHIFT, SA_KEY_MASK);
                hi = sa_lower_bound(tfp + base, lo, df, (d0 + (u64)TILE) << SA_KEY_SHIFT, SA_KEY_MASK);
            }
            first = sa_imp_base(base, term) + lo;
            cnt = hi - lo;
        }
        s_first[tid] = first; s_cnt[tid] = cnt;
    }
    __syncthreads();
    for (u32 t = 0; t < T; t++) {                               // (uniform)
        const u64 first = s_first[t];
        const u32 cnt = s_cnt[t];
        const float w = q.w[t];
        for (u32 j = tid; j < cnt; j += 256u) {
            const u64 cell = imp[first + j];
            const u32 d = ((u32)(cell >> 32) >> 2) - (u32)d0;   // (a term holds a doc once: no two lanes meet on an accumulator)
            acc[d] = __fadd_rn(acc[d], __fmul_rn(__uint_as_float((u32)cell), w));
        }
        if (T > 1u) __syncthreads();
    }
    __syncthreads();
    const u64 left = n_docs - d0;
    const u32 n = left < (u64)TILE ? (u32)left : (u32)TILE;
    if (n == (u32)TILE && (n_docs & 3ull) == 0ull) {
        for (u32 i = tid; i < (u32)TILE / 4u; i += 256u) {
            float4 v = ((const float4*)acc)[i];
            if (has_boost) { v.x = __fmul_rn(v.x, boost); v.y = __fmul_rn(v.y, boost); v.z = __fmul_rn(v.z, boost); v.w = __fmul_rn(v.w, boost); }
            ((float4*)(out + d0))[i] = v;
        }
    } else {
        for (u32 i = tid; i < n; i += 256u) out[d0 + i] = has_boost ? __fmul_rn(acc[i], boost) : acc[i];
    }
}

extern "C" int sa_index_bm25_dense(sa_index_t* ix, const uint32_t* terms, const float* idf,
                                   int n_query_terms, float k1, float b, float* out) {
    SA_ARG(ix && out, "null argument");
    SA_ARG(n_query_terms >= 0, "n_query_terms < 0");
    SA_ARG(n_query_terms == 0 || (terms && idf), "terms/idf null");
    std::unique_lock<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    SaDenseLaneScope lane(ix, g);                               // (enqueue under the lock, wait outside it: sa_index.hpp, DenseLane)
    SA_TRY(lane.rc);
    hipStream_t st = ix->stream;
    const u64 N = ix->n_docs;
    // reference similarity.py:31-32: avg_doc_lens == 0 -> zeros
    if (N == 0 || n_query_terms == 0 || ix->avg_doc_len == 0.f) {
        sa_emit_zeros(ix, out);
        return SA_OK;
    }
    const int T = n_query_terms;
    SA_ARG(T <= SA_MAX_QTERMS, "more than 32 query terms per call is not supported");
    // One launch over the impact stream of (k1, b) -- the stream the index already holds for these parameters, or a new one when
    // it holds none (built once: the batches of the same parameters share it); an index whose stream belongs to OTHER parameters
    // keeps it and scores the TF postings as before.
    if (sa_opt(ix->opts.dense_direct, 1) != 0 && (ix->tile_docs == 1024 || ix->tile_docs == 2048 || ix->tile_docs == 4096) && ix->n_tiles > 0) {
        auto same = [](float x, float y) { return memcmp(&x, &y, sizeof(float)) == 0; };
        std::shared_ptr<sa_impacts> im;
        if (!ix->impacts || (same(ix->impacts->k1, k1) && same(ix->impacts->b, b) && same(ix->impacts->avgdl, ix->avg_doc_len)))
            im = sa_impacts_get(ix, k1, b, ix->opts);
        if (im && im->d_imp) {
            DenseQuery dq;
            memset(&dq, 0, sizeof(dq));
            for (int i = 0; i < T; i++) { dq.term[i] = terms[i]; dq.w[i] = idf[i]; }
            float* dst = nullptr; float boost = 1.f; int has_boost = 0;
            const bool to_vec = sa_vec_target_take(ix, &dst, &boost, &has_boost);
            if (!to_vec) {
                void* scratch;
                SA_TRY(sa_index_scratch(ix, N * sizeof(float) + 1024, &scratch));
                dst = (float*)scratch;
            }
#define SA_LAUNCH_DENSE(TILE)                                                                                                      \
    hipLaunchKernelGGL((sa_k_bm25_dense_direct<TILE>), dim3(ix->n_tiles), dim3(256), 0, st, (const u64*)ix->d_tfp, (const u64*)ix->d_tf_off, \
                       (const u32*)ix->d_dir_slot, (const u32*)ix->d_tile_dir, (const u64*)im->d_imp, ix->n_terms, ix->n_tiles, N, dq, (u32)T,  \
                       boost, has_boost, dst)
            if (ix->tile_docs == 1024) SA_LAUNCH_DENSE(1024);
            else if (ix->tile_docs == 2048) SA_LAUNCH_DENSE(2048);
            else SA_LAUNCH_DENSE(4096);
#undef SA_LAUNCH_DENSE
            SA_HIP(hipGetLastError());
            if (!to_vec) SA_TRY(sa_emit_dense(ix, dst, out));
            SA_TRY(lane.finish());
            return SA_OK;
        }
    }
    // scratch: [out chunk accumulators N floats][terms][idf]
    void* scratch;
    const size_t nb = (size_t)T * (ix->n_tiles + 1);
    SA_TRY(sa_index_scratch(ix, N * sizeof(float) + (size_t)T * 16 + nb * 4 + SA_SAT_NTF * SA_SAT_WMAX * 4 + 1024, &scratch));
    float* d_out = (float*)scratch;
    u64* d_qbase = (u64*)(d_out + ((N + 1) & ~(u64)1));
    u32* d_terms = (u32*)(d_qbase + T);
    float* d_idf = (float*)(d_terms + T);
    float* d_tab = d_idf + T;
    u32* d_bounds = (u32*)(d_tab + SA_SAT_NTF * SA_SAT_WMAX);
    SA_HIP(hipMemcpyAsync(d_terms, terms, (size_t)T * sizeof(u32), hipMemcpyHostToDevice, st));
    SA_HIP(hipMemcpyAsync(d_idf, idf, (size_t)T * sizeof(float), hipMemcpyHostToDevice, st));
    Bm25Params p;
    memset(&p, 0, sizeof(p));
    sa_fill_params(ix, p);
    p.terms = d_terms; p.idf = d_idf; p.B = 1; p.nq = 1; p.T = (u32)T; p.k = 0;
    p.k1 = k1; p.b = b; p.pruned = 0;
    p.dense_out = d_out; p.cand = nullptr;
    p.bounds = d_bounds; p.qbase = d_qbase;
    p.sattab = d_tab;
    SA_TRY(sa_launch_make_sattab(ix, d_tab, &p.tab_w, k1, b, st));
    SA_TRY(sa_launch_make_bounds(ix, d_terms, (u32)T, d_bounds, d_qbase, st));
    SA_TRY(sa_launch_bm25(ix, p, st));
    SA_TRY(sa_emit_dense(ix, d_out, out));
    SA_TRY(lane.finish());
    SA_HIP(hipGetLastError());
    return SA_OK;
}


// regroup an all-gather result [rank][B*k (+ extra)] into per-query candidate rows [B][rank*k]; `extra` = 1: every
// rank's block ends with its overflow flag, OR-ed into *xflag (a candidate list ran over on SOME rank: all ranks
// learn it from the exchange itself and redo the batch together at fetch)
__global__ void sa_k_regroup(const u64* __restrict__ gathered, u32 nranks, u32 B, u32 k, u32 extra, u64* __restrict__ out,
                             u32* __restrict__ xflag) {
    const u64 per = (u64)B * k;
    const u64 total = (u64)nranks * per;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (u64)gridDim.x * blockDim.x) {
        const u32 j = (u32)(i % k);
        const u32 q = (u32)((i / k) % B);
        const u32 r = (u32)(i / per);
        out[((u64)q * nranks + r) * k + j] = gathered[(u64)r * (per + extra) + (i - (u64)r * per)];
    }
    if (extra && xflag && blockIdx.x == 0 && threadIdx.x == 0) {
        u32 any = 0;
        for (u32 r = 0; r < nranks; r++) any |= gathered[(u64)r * (per + extra) + per] != 0ull ? 1u : 0u;
        if (any) *xflag = 1u;
    }
}

void sa_launch_regroup(const u64* gathered, u32 nranks, u32 B, u32 k, u32 extra, u64* out, u32* xflag, hipStream_t st) {
    const u64 total = (u64)nranks * B * k;
    const u32 grid = total / 256 + 1 < 4096 ? (u32)(total / 256 + 1) : 4096;
    hipLaunchKernelGGL(sa_k_regroup, dim3(grid), dim3(256), 0, st, gathered, nranks, B, k, extra, out, xflag);
}

void sa_launch_topk_merge(u32 B, hipStream_t st, u64* cand, u32 n_cand_max, u32 k, u64* out, const u32* out_row, u32 rank_stride,
                          const u32* cnt, const u32* slots, const u32* gthr, u32* overflow, u32* clr_state, u32 clr_B, u32 clr_hist,
                          u32* clr_one, u32 gather_stride, u32* xflag, const u32* seed) {
    if (k <= 64u)
        hipLaunchKernelGGL(sa_k_topk_merge<256>, dim3(B), dim3(256), 0, st, cand, n_cand_max, k, out, out_row, rank_stride, cnt, slots,
                           gthr, overflow, clr_state, clr_B, clr_hist, clr_one, gather_stride, xflag, seed);
    else
        hipLaunchKernelGGL(sa_k_topk_merge<1024>, dim3(B), dim3(1024), 0, st, cand, n_cand_max, k, out, out_row, rank_stride, cnt, slots,
                           gthr, overflow, clr_state, clr_B, clr_hist, clr_one, gather_stride, xflag, seed);
}
