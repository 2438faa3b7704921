// sa_facet.hip -- Part 2d of the C ABI: a device column of category codes (sa_codes_create / sa_codes_destroy) and the facet counts
// of a dense device vector (sa_vec_facet_counts) -- how a multi-field query (searcharray_amd.solr.edismax_facets) gets its hit count
// and its counts per category without copying its n scores to the host.  The facet counts of a BM25 batch
// (sa_batch_facet_counts) use the same column: their host code is in sa_batch.hip, their kernel beside the tile item in sa_bm25.hip.
#include "sa_facet.hpp"
#include "sa_vec.hpp"
#include "sa_filter.hpp"
#include "../../include/searcharray_hip.h"

#include <new>
#include <vector>

#define SA_VFC_TILE 1024u                        // entries per workgroup iteration == SA_FILTER_BLOCK
#define SA_VFC_THREADS 256
#define SA_VFC_MAX_GRID 2048u

static_assert(SA_VFC_TILE == SA_FILTER_BLOCK, "a tile is one block of the filter summary");

extern "C" int sa_codes_create(sa_index_t* ix, const int32_t* codes, uint64_t n_docs, uint32_t n_values, sa_codes_t** out) {
    SA_ARG(ix && out && (codes || n_docs == 0), "null argument");
    SA_ARG(n_docs == ix->n_docs, "a column has one code per document of the index");
    SA_ARG(n_values >= 1 && n_values <= SA_FACET_MAX_VALUES, "n_values must be in 1 .. 2^20");
    for (u64 i = 0; i < n_docs; i++)
        SA_ARG(codes[i] >= -1 && codes[i] < (int64_t)n_values, "codes must be -1 (no value) or in [0, n_values)");
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    sa_codes* c = new (std::nothrow) sa_codes();
    if (!c) { sa_set_error("out of host memory"); return SA_ERR_NOMEM; }
    c->device = ix->device; c->n_docs = n_docs; c->n_values = n_values;
    const size_t bytes = (size_t)(n_docs ? n_docs : 1) * sizeof(int);
    if (hipMalloc(&c->d, bytes) != hipSuccess) { (void)hipGetLastError(); delete c; sa_set_error("hipMalloc failed (column of codes)"); return SA_ERR_HIP; }
    if ((n_docs && hipMemcpyAsync(c->d, codes, (size_t)n_docs * sizeof(int), hipMemcpyHostToDevice, ix->stream) != hipSuccess) ||
        hipStreamSynchronize(ix->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(c->d); delete c;
        sa_set_error("sa_codes_create: the upload failed");
        return SA_ERR_HIP;
    }
    *out = c;
    return SA_OK;
}

extern "C" int sa_codes_destroy(sa_codes_t* c) {
    if (!c) return SA_OK;
    if (c->d) { (void)hipSetDevice(c->device); (void)hipFree(c->d); }
    delete c;
    return SA_OK;
}

// One streaming pass over the vector.  A workgroup walks 1024-entry tiles (one block of the filter's summary each; blocks the summary
// counts empty are not read): an entry counts when its value is > 0 (NaN never is) and its filter bit is set -- sa_vec_topk's
// eligibility.  Consecutive lanes read consecutive values and codes.  Columns of up to SA_FACET_LDS_BINS values are counted in an LDS
// histogram the workgroup keeps across ALL its tiles and adds to the global counters once, one atomic per non-zero bin; larger
// columns bump the global counters directly.  out2: [0] found, [1] missing.
template <bool F64>
__global__ void __launch_bounds__(SA_VFC_THREADS)
sa_k_vec_facet(const void* __restrict__ data, u64 n, const u32* __restrict__ fwords, const u32* __restrict__ fblk, u32 tile0, u32 n_tiles,
               const int* __restrict__ codes, u32 n_values, u32* __restrict__ counts, u32* __restrict__ out2) {
    constexpr int NW = SA_VFC_THREADS / SA_WAVE;
    __shared__ u32 h[SA_FACET_LDS_BINS];
    __shared__ u32 red[NW + 1];
    const u32 tid = threadIdx.x;
    const bool lds = codes != nullptr && n_values <= SA_FACET_LDS_BINS;      // (uniform)
    if (lds) {
        for (u32 i = tid; i < n_values; i += SA_VFC_THREADS) h[i] = 0u;
        __syncthreads();
    }
    u32 found = 0, miss = 0;
    for (u32 tile = tile0 + blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (fblk && fblk[tile] == 0u) continue;                               // (uniform) nothing eligible in this block
        const u64 base = (u64)tile * SA_VFC_TILE;
#pragma unroll
        for (u32 j = 0; j < SA_VFC_TILE / SA_VFC_THREADS; j++) {
            const u64 i = base + j * SA_VFC_THREADS + tid;
            if (i >= n) continue;
            const bool pos = F64 ? ((const double*)data)[i] > 0.0 : ((const float*)data)[i] > 0.f;
            if (!pos) continue;
            if (fwords && !((fwords[i >> 5] >> (u32)(i & 31u)) & 1u)) continue;
            found++;
            if (codes) {
                const int c = codes[i];
                if (c < 0) miss++;
                else if (lds) atomicAdd(&h[c], 1u);
                else atomicAdd(&counts[c], 1u);
            }
        }
    }
    const u32 f = sa_block_sum<NW>(found, red);
    const u32 m = sa_block_sum<NW>(miss, red);                                // (its barriers: every bump of the histogram is done)
    if (f == 0u) return;                                                      // (uniform)
    if (tid == 0) {
        atomicAdd(&out2[0], f);
        if (m) atomicAdd(&out2[1], m);
    }
    if (lds) {
        for (u32 i = tid; i < n_values; i += SA_VFC_THREADS) {
            const u32 c = h[i];
            if (c) atomicAdd(&counts[i], c);
        }
    }
}

extern "C" int sa_vec_facet_counts(sa_vec_t* v, sa_filter_t* filter, sa_codes_t* codes, uint64_t* found_out, uint64_t* missing_out,
                                   uint32_t* counts_out) {
    SA_ARG(v && found_out, "null argument");
    SA_ARG(v->n < (1ull << 32), "vector too long (the counters are 32 bits wide)");
    const sa_filter_data* f = nullptr;
    if (filter) {
        SA_ARG(filter->d, "null filter");
        f = filter->d.get();
        SA_ARG(f->device == v->device, "the filter lives on another device than the vector");
        SA_ARG(f->n_docs == v->n, "the filter covers another number of documents than the vector holds");
    }
    const size_t V = codes ? codes->n_values : 0;
    if (codes) {
        SA_ARG(missing_out && counts_out, "missing_out / counts_out null with a column");
        SA_ARG(codes->device == v->device, "the column lives on another device than the vector");
        SA_ARG(codes->n_docs == v->n, "the column covers another number of documents than the vector holds");
    }
    *found_out = 0;
    if (codes) {
        *missing_out = 0;
        memset(counts_out, 0, V * sizeof(u32));
    }
    const u32 n_tiles = (u32)((v->n + SA_VFC_TILE - 1u) / SA_VFC_TILE);
    const u32 tile0 = f ? f->first_block : 0u;
    if (v->n == 0 || tile0 >= n_tiles) return SA_OK;                          // nothing eligible: nothing is read
    SA_HIP(hipSetDevice(v->device));
    hipStream_t st = sa_vec_stream(v->device);
    u32* d_cnt = nullptr;                                                     // [2] found, missing | [V] counts
    SA_HIP(hipMalloc(&d_cnt, (2 + V) * sizeof(u32)));
    std::vector<u32> h2(2, 0u);
    const u32 grid = n_tiles - tile0 < SA_VFC_MAX_GRID ? n_tiles - tile0 : SA_VFC_MAX_GRID;
    const u32* fwords = f ? (const u32*)f->d_words : nullptr;
    const u32* fblk = f ? (const u32*)f->d_blk : nullptr;
    bool ok = hipMemsetAsync(d_cnt, 0, (2 + V) * sizeof(u32), st) == hipSuccess;
    if (ok) {
        if (v->f64) hipLaunchKernelGGL((sa_k_vec_facet<true>), dim3(grid), dim3(SA_VFC_THREADS), 0, st, (const void*)v->d, v->n, fwords, fblk, tile0,
                                       n_tiles, codes ? (const int*)codes->d : (const int*)nullptr, (u32)V, d_cnt + 2, d_cnt);
        else hipLaunchKernelGGL((sa_k_vec_facet<false>), dim3(grid), dim3(SA_VFC_THREADS), 0, st, (const void*)v->d, v->n, fwords, fblk, tile0,
                                n_tiles, codes ? (const int*)codes->d : (const int*)nullptr, (u32)V, d_cnt + 2, d_cnt);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(h2.data(), d_cnt, 2 * sizeof(u32), hipMemcpyDeviceToHost, st) == hipSuccess &&
             (!V || hipMemcpyAsync(counts_out, d_cnt + 2, V * sizeof(u32), hipMemcpyDeviceToHost, st) == hipSuccess);
    }
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    (void)hipFree(d_cnt);
    if (!ok) { (void)hipGetLastError(); sa_set_error("sa_vec_facet_counts: the counting pass failed"); return SA_ERR_HIP; }
    *found_out = h2[0];
    if (codes) *missing_out = h2[1];
    return SA_OK;
}
