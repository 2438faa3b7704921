// sa_filter.hip -- Part 2b of the C ABI: document filters of an index (sa_filter.hpp).  A filter is built on the index stream from
// doc ids, a byte mask or a term's postings, combined word by word with others of the same index, and handed to a BM25 batch
// (sa_batch_set_filter, sa_batch.hip), whose kernels rank inside it.  Small grid-stride kernels; nothing here is on the hot path.
#include "sa_filter.hpp"
#include "../../include/searcharray_hip.h"

#include <new>
#include <vector>

sa_filter_data::~sa_filter_data() {
    if (d_words || d_blk) (void)hipSetDevice(device);
    if (d_words) (void)hipFree(d_words);
    if (d_blk) (void)hipFree(d_blk);
}

// doc ids (global: doc_base is subtracted, ids outside the shard are ignored) -> bits
__global__ void __launch_bounds__(256)
sa_k_filter_rows(const u64* __restrict__ ids, u64 n, u64 doc_base, u64 n_docs, u32* __restrict__ bits) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 d = ids[i] - doc_base;                        // (an id below the base wraps far beyond n_docs)
        if (d < n_docs) atomicOr(&bits[d >> 5], 1u << (u32)(d & 31u));
    }
}

// one byte per doc, non-zero = eligible: a thread forms one 32-bit word
__global__ void __launch_bounds__(256)
sa_k_filter_mask(const unsigned char* __restrict__ mask, u64 n_docs, u32* __restrict__ bits) {
    const u64 n32 = (n_docs + 31u) >> 5;
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < n32; w += (u64)gridDim.x * blockDim.x) {
        u32 v = 0;
        for (u32 j = 0; j < 32u; j++) {
            const u64 d = (w << 5) + j;
            if (d < n_docs && mask[d]) v |= 1u << j;
        }
        bits[w] = v;
    }
}

// the docs of a term's TF postings [lo, hi)
__global__ void __launch_bounds__(256)
sa_k_filter_term(const u64* __restrict__ tfp, u64 lo, u64 hi, u64 n_docs, u32* __restrict__ bits) {
    for (u64 i = lo + (u64)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (u64)gridDim.x * blockDim.x) {
        const u64 d = tfp[i] >> SA_KEY_SHIFT;
        if (d < n_docs) atomicOr(&bits[d >> 5], 1u << (u32)(d & 31u));
    }
}

// out = a op b over the n_words words that cover the docs (op 3: ~a); the last word keeps its tail bits 0
__global__ void __launch_bounds__(256)
sa_k_filter_combine(const u64* __restrict__ a, const u64* __restrict__ b, int op, u64 n_words, u64 tail_mask, u64* __restrict__ out) {
    for (u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (u64)gridDim.x * blockDim.x) {
        const u64 x = a[w], y = b ? b[w] : 0ull;
        u64 r = op == SA_FILTER_AND ? (x & y) : op == SA_FILTER_OR ? (x | y) : op == SA_FILTER_ANDNOT ? (x & ~y) : ~x;
        if (w + 1u == n_words) r &= tail_mask;
        out[w] = r;
    }
}

// blk[i] = eligible docs of block i (the cell behind the last block: 0)
__global__ void __launch_bounds__(256)
sa_k_filter_summary(const u64* __restrict__ words, u32 n_cells, u32* __restrict__ blk) {
    constexpr u32 WPB = SA_FILTER_BLOCK / 64u;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += gridDim.x * blockDim.x) {
        u32 c = 0;
        for (u32 j = 0; j < WPB; j++) c += (u32)__popcll((unsigned long long)words[(u64)i * WPB + j]);
        blk[i] = c;
    }
}

static u32 sa_filter_grid(u64 items) {
    const u64 g = (items + 255u) / 256u;
    return (u32)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

// an all-zero filter of `ix` (enqueued on the index stream; call with the index lock held)
static int sa_filter_alloc(sa_index* ix, std::shared_ptr<sa_filter_data>* out) {
    std::shared_ptr<sa_filter_data> f(new (std::nothrow) sa_filter_data());
    if (!f) { sa_set_error("out of host memory"); return SA_ERR_NOMEM; }
    f->ix = ix; f->device = ix->device; f->n_docs = ix->n_docs;
    f->n_words = (ix->n_docs + 63u) >> 6;
    f->n_blocks = (u32)((ix->n_docs + SA_FILTER_BLOCK - 1u) / SA_FILTER_BLOCK);
    // whole blocks, and one more: a kernel may read the words of a whole tile (staged route: up to 16) from any 64-doc boundary inside the shard
    f->n_alloc = ((u64)f->n_blocks + 1u) * (SA_FILTER_BLOCK / 64u);
    SA_HIP(hipMalloc(&f->d_words, f->n_alloc * sizeof(u64)));
    SA_HIP(hipMalloc(&f->d_blk, ((size_t)f->n_blocks + 1u) * sizeof(u32)));
    SA_HIP(hipMemsetAsync(f->d_words, 0, f->n_alloc * sizeof(u64), ix->stream));
    *out = f;
    return SA_OK;
}

// summary + count; the filter is complete when this returns
static int sa_filter_finish(sa_index* ix, const std::shared_ptr<sa_filter_data>& f, sa_filter_t** out) {
    const u32 cells = f->n_blocks + 1u;
    hipLaunchKernelGGL(sa_k_filter_summary, dim3(sa_filter_grid(cells)), dim3(256), 0, ix->stream, (const u64*)f->d_words, cells, f->d_blk);
    SA_HIP(hipGetLastError());
    std::vector<u32> h(cells);
    SA_HIP(hipMemcpyAsync(h.data(), f->d_blk, (size_t)cells * sizeof(u32), hipMemcpyDeviceToHost, ix->stream));
    SA_HIP(hipStreamSynchronize(ix->stream));
    f->count = 0;
    f->first_block = f->n_blocks;
    for (u32 i = 0; i < cells; i++) {
        f->count += h[i];
        if (h[i] && f->first_block == f->n_blocks) f->first_block = i;
    }
    sa_filter* h_out = new (std::nothrow) sa_filter();
    if (!h_out) { sa_set_error("out of host memory"); return SA_ERR_NOMEM; }
    h_out->d = f;
    *out = h_out;
    return SA_OK;
}

extern "C" int sa_filter_create_from_rows(sa_index_t* ix, const uint64_t* doc_ids, uint64_t n, sa_filter_t** out) {
    SA_ARG(ix && out && (doc_ids || n == 0), "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    std::shared_ptr<sa_filter_data> f;
    SA_TRY(sa_filter_alloc(ix, &f));
    if (n && ix->n_docs) {
        u64* d_ids = nullptr;
        SA_HIP(hipMalloc(&d_ids, (size_t)n * sizeof(u64)));
        int rc = SA_OK;
        if (hipMemcpyAsync(d_ids, doc_ids, (size_t)n * sizeof(u64), hipMemcpyHostToDevice, ix->stream) != hipSuccess) rc = SA_ERR_HIP;
        if (rc == SA_OK) {
            hipLaunchKernelGGL(sa_k_filter_rows, dim3(sa_filter_grid(n)), dim3(256), 0, ix->stream, (const u64*)d_ids, (u64)n, ix->doc_base,
                               ix->n_docs, (u32*)f->d_words);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) rc = SA_ERR_HIP;
        }
        (void)hipFree(d_ids);
        if (rc != SA_OK) { sa_set_error("sa_filter_create_from_rows: the upload or the scatter kernel failed"); return rc; }
    }
    return sa_filter_finish(ix, f, out);
}

extern "C" int sa_filter_create_from_mask(sa_index_t* ix, const uint8_t* mask, uint64_t n_docs, sa_filter_t** out) {
    SA_ARG(ix && out && (mask || n_docs == 0), "null argument");
    SA_ARG(n_docs == ix->n_docs, "a filter mask has one byte per document of the index");
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    std::shared_ptr<sa_filter_data> f;
    SA_TRY(sa_filter_alloc(ix, &f));
    if (n_docs) {
        unsigned char* d_mask = nullptr;
        SA_HIP(hipMalloc(&d_mask, (size_t)n_docs));
        int rc = SA_OK;
        if (hipMemcpyAsync(d_mask, mask, (size_t)n_docs, hipMemcpyHostToDevice, ix->stream) != hipSuccess) rc = SA_ERR_HIP;
        if (rc == SA_OK) {
            hipLaunchKernelGGL(sa_k_filter_mask, dim3(sa_filter_grid((n_docs + 31u) >> 5)), dim3(256), 0, ix->stream, (const unsigned char*)d_mask,
                               (u64)n_docs, (u32*)f->d_words);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->stream) != hipSuccess) rc = SA_ERR_HIP;
        }
        (void)hipFree(d_mask);
        if (rc != SA_OK) { sa_set_error("sa_filter_create_from_mask: the upload or the pack kernel failed"); return rc; }
    }
    return sa_filter_finish(ix, f, out);
}

extern "C" int sa_filter_create_from_term(sa_index_t* ix, uint32_t term, sa_filter_t** out) {
    SA_ARG(ix && out, "null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    std::shared_ptr<sa_filter_data> f;
    SA_TRY(sa_filter_alloc(ix, &f));
    if (term < ix->n_terms) {                                   // (an unknown term: the empty filter)
        const u64 lo = ix->h_tf_off[term], hi = ix->h_tf_off[(size_t)term + 1];
        if (hi > lo) {
            hipLaunchKernelGGL(sa_k_filter_term, dim3(sa_filter_grid(hi - lo)), dim3(256), 0, ix->stream, (const u64*)ix->d_tfp, lo, hi, ix->n_docs,
                               (u32*)f->d_words);
            SA_HIP(hipGetLastError());
        }
    }
    return sa_filter_finish(ix, f, out);
}

static int sa_filter_combine_impl(sa_filter_t* a, sa_filter_t* b, int op, sa_filter_t** out) {
    const sa_filter_data* fa = a->d.get();
    sa_index* ix = const_cast<sa_index*>(fa->ix);
    std::lock_guard<std::mutex> g(ix->mu);
    SA_HIP(hipSetDevice(ix->device));
    std::shared_ptr<sa_filter_data> f;
    SA_TRY(sa_filter_alloc(ix, &f));
    if (f->n_words) {
        const u32 tail = (u32)(f->n_docs & 63u);
        const u64 tail_mask = tail ? (1ull << tail) - 1ull : ~0ull;
        hipLaunchKernelGGL(sa_k_filter_combine, dim3(sa_filter_grid(f->n_words)), dim3(256), 0, ix->stream, (const u64*)fa->d_words,
                           b ? (const u64*)b->d->d_words : (const u64*)nullptr, op, f->n_words, tail_mask, f->d_words);
        SA_HIP(hipGetLastError());
    }
    return sa_filter_finish(ix, f, out);
}

extern "C" int sa_filter_combine(sa_filter_t* a, sa_filter_t* b, int op, sa_filter_t** out) {
    SA_ARG(a && b && out && a->d && b->d, "null argument");
    SA_ARG(op == SA_FILTER_AND || op == SA_FILTER_OR || op == SA_FILTER_ANDNOT, "op must be SA_FILTER_AND, SA_FILTER_OR or SA_FILTER_ANDNOT");
    SA_ARG(a->d->ix == b->d->ix && a->d->n_docs == b->d->n_docs, "the two filters belong to different indexes");
    return sa_filter_combine_impl(a, b, op, out);
}

extern "C" int sa_filter_not(sa_filter_t* a, sa_filter_t** out) {
    SA_ARG(a && out && a->d, "null argument");
    return sa_filter_combine_impl(a, nullptr, 3, out);
}

extern "C" int sa_filter_count(sa_filter_t* f, uint64_t* n_out) {
    SA_ARG(f && f->d && n_out, "null argument");
    *n_out = f->d->count;
    return SA_OK;
}

extern "C" int sa_filter_fetch(sa_filter_t* f, uint8_t* mask_out) {
    SA_ARG(f && f->d && (mask_out || f->d->n_docs == 0), "null argument");
    const sa_filter_data* d = f->d.get();
    std::vector<u64> h((size_t)d->n_words);
    if (d->n_words) {
        SA_HIP(hipSetDevice(d->device));
        SA_HIP(hipMemcpy(h.data(), d->d_words, (size_t)d->n_words * sizeof(u64), hipMemcpyDeviceToHost));
    }
    for (u64 i = 0; i < d->n_docs; i++) mask_out[i] = (uint8_t)((h[(size_t)(i >> 6)] >> (i & 63u)) & 1u);
    return SA_OK;
}

extern "C" int sa_filter_destroy(sa_filter_t* f) {
    delete f;                                                   // (the bitmap lives on while a batch holds it)
    return SA_OK;
}
