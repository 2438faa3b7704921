// sa_vec_topk.hip -- Part 4 of the C ABI: the k best entries of a dense device vector (sa_vec_topk), optionally inside a document
// filter, and the host -> vector copy (sa_vec_store).  This is how a multi-field query (searcharray_amd.solr.edismax_search) ends:
// the combined scores never leave HBM, k values and k indices do.
//
// The ranking key of entry i with value v > 0 is the pair (bits of v, i): a non-negative IEEE value is monotone as an unsigned
// integer, float64 keeps all 64 bits (nothing is rounded to select), and "value descending, then index ascending" is the descending
// order of the integer   key = bits(v) << IB | (2^IB - 1 - i)   with IB = the bits an index below n needs.  Keys are unique.
//
// Selection = MSB-first radix select on that key, 12 bits a level, every level one streaming pass over the vector:
//   pass     reads the vector once (16-byte loads, one 1024-entry tile = one filter block per workgroup iteration; blocks the filter's
//            summary counts empty are not read) and, for the entries whose key matches the prefix found so far, counts the next
//            digit in a 4096-bin LDS histogram that is added to a global one with integer atomics (order-independent).  The same
//            pass appends to the candidate list every entry the PREVIOUS level proved to be above the boundary bin.
//   find     one workgroup: the bin that holds the k-th largest key, how many entries lie above it, and whether the boundary bin
//            fits the candidate list with them.  If it does, the next pass appends it and is the last; else the next level
//            refines INSIDE the boundary bin -- down into the index bits when the values tie (a constant vector) --, so the number
//            of passes is bounded by the key width, ceil((63 or 31 + IB) / 12) + 1, never by the data.
//   final    one workgroup sorts the candidates (at most 4096 pairs in LDS, bitonic, pair comparison) and writes the first k.
// All decisions live in a small state block in device memory, so the host enqueues passes without reading anything back; one
// device-to-host copy returns state, values and indices.  The result is a pure function of (vector, filter, k): histogram sums do
// not depend on the order of the atomics, and the order in which candidates are appended is erased by the final sort.
#include "sa_vec.hpp"
#include "sa_filter.hpp"
#include "../../include/searcharray_hip.h"
#include <new>
#include <vector>

typedef unsigned __int128 u128;

#define SA_VTK_BITS 12
#define SA_VTK_BINS (1u << SA_VTK_BITS)
#define SA_VTK_CAP 4096u                         // candidate list (pairs); >= SA_KMAX + one boundary bin worth keeping
#define SA_VTK_TILE 1024u                        // entries per workgroup iteration == SA_FILTER_BLOCK
#define SA_VTK_THREADS 256
#define SA_VTK_KMAX 1024u                        // == SA_KMAX of the batches (sa_batch.hpp)
#define SA_VTK_MAX_GRID 2048u                    // 256 CUs x 8 resident workgroups of 4 waves

static_assert(SA_VTK_TILE == SA_FILTER_BLOCK, "a tile is one block of the filter summary");
static_assert(SA_VTK_KMAX < SA_VTK_CAP, "the entries above the boundary bins (fewer than k) and a last bin of one entry fit the list");

struct sa_vtk_state {
    u64 bound_hi, bound_lo;                      // key >> bound_p of the boundary bin found last (prefix and digit)
    unsigned long long found;                    // eligible entries (counted by the first pass)
    u32 level;                                   // the level the next pass counts
    u32 have_bound, bound_p, prev_s;             // prev_s: the new bits the last digit added to the prefix
    u32 append_bin;                              // the next pass appends the boundary bin too and is the last
    u32 take_all;                                // the next pass appends every eligible entry and is the last
    u32 done;
    u32 k_rem;                                   // entries still to take from the boundary bin
    u32 cand_cnt;
    u32 passes;                                  // passes that did work
    u32 pad_[16];
};
static_assert(sizeof(sa_vtk_state) == 128, "state block");

struct sa_vec_topk_scratch {
    char* d = nullptr;                           // one allocation: hist | state | out | cand_val | cand_idx
    u32* hist = nullptr;
    sa_vtk_state* st = nullptr;
    u64* out = nullptr;                          // [k][2]: value bits, index
    u64* cand_val = nullptr;
    u64* cand_idx = nullptr;
    std::vector<u64> host;                       // state + out, as copied back
    int passes = 0;
};

void sa_vec_topk_release(sa_vec* v) {
    if (!v->topk) return;
    if (v->topk->d) (void)hipFree(v->topk->d);
    delete v->topk;
    v->topk = nullptr;
}

// shift of the digit of `level` in a key of `tb` bits (the last level overlaps the one before it: those bits are fixed by then)
__host__ __device__ static inline int sa_vtk_shift(int tb, int level) {
    const int p = tb - SA_VTK_BITS * (level + 1);
    return p > 0 ? p : 0;
}

// ---- pass: count the next digit inside the prefix, append what the last level decided ------------------------------------------
template <bool F64>
__global__ void __launch_bounds__(SA_VTK_THREADS)
sa_k_vec_topk_pass(const void* __restrict__ data, u64 n, const u32* __restrict__ fwords, const u32* __restrict__ fblk, u32 tile0,
                   u32 n_tiles, int ib, sa_vtk_state* __restrict__ st, u32* __restrict__ ghist, u64* __restrict__ cand_val,
                   u64* __restrict__ cand_idx) {
    __shared__ u32 h[SA_VTK_BINS];
    if (st->done) return;
    const u32 level = st->level, have_bound = st->have_bound, append_bin = st->append_bin, take_all = st->take_all;
    const int tb = (F64 ? 63 : 31) + ib;
    const int p = sa_vtk_shift(tb, (int)level), pp = (int)st->bound_p, prev_s = (int)st->prev_s;
    const u128 bound = ((u128)st->bound_hi << 64) | (u128)st->bound_lo;
    const bool counting = !(append_bin || take_all);
    const u64 imask = (1ull << ib) - 1ull;
    const u64 vmax = F64 ? 0x7FF0000000000000ull : 0x7F800000ull;        // +inf: the largest value that ranks (NaN lies above)
    const u32 tid = threadIdx.x, lane = tid & (SA_WAVE - 1);
    const u64 lt = (1ull << lane) - 1ull;
    if (counting) {
        for (u32 i = tid; i < SA_VTK_BINS; i += SA_VTK_THREADS) h[i] = 0;
        __syncthreads();
    }
    u32 n_elig = 0;
    for (u32 tile = tile0 + blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if (fblk && fblk[tile] == 0) continue;                            // (workgroup-uniform) nothing eligible in this block
        const u64 base = (u64)tile * SA_VTK_TILE;
        u64 val[4], idx[4];
#pragma unroll
        for (int j = 0; j < 4; j++) idx[j] = F64 ? base + (u64)(j >> 1) * 512u + 2u * tid + (u64)(j & 1) : base + 4u * tid + (u64)j;
        if (base + SA_VTK_TILE <= n) {
            if (F64) {
                const uint4 a = ((const uint4*)data)[(base >> 1) + tid], b = ((const uint4*)data)[(base >> 1) + 256u + tid];
                val[0] = (u64)a.x | ((u64)a.y << 32); val[1] = (u64)a.z | ((u64)a.w << 32);
                val[2] = (u64)b.x | ((u64)b.y << 32); val[3] = (u64)b.z | ((u64)b.w << 32);
            } else {
                const uint4 a = ((const uint4*)data)[(base >> 2) + tid];
                val[0] = a.x; val[1] = a.y; val[2] = a.z; val[3] = a.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                val[j] = idx[j] < n ? (F64 ? ((const u64*)data)[idx[j]] : (u64)((const u32*)data)[idx[j]]) : 0ull;
        }
        if (fwords) {                                                     // (the bitmap covers whole blocks: no bound to check)
            const u32 w0 = fwords[idx[0] >> 5], w2 = fwords[idx[2] >> 5];
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (!(((j < 2 ? w0 : w2) >> (u32)(idx[j] & 31u)) & 1u)) val[j] = 0ull;
        }
        // class of every entry: 0 nothing, 1 append, 2 count digit dg
        u32 cls[4], dg[4];
        u32 n_app = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            cls[j] = 0; dg[j] = 0;
            if (val[j] != 0ull && val[j] <= vmax) {
                n_elig++;
                const u128 key = ((u128)val[j] << ib) | (u128)(imask - idx[j]);
                dg[j] = (u32)(key >> p) & (SA_VTK_BINS - 1u);
                if (take_all) cls[j] = 1;
                else if (!have_bound) cls[j] = 2;
                else {
                    const u128 x = key >> pp;
                    if (x == bound) cls[j] = append_bin ? 1u : 2u;
                    else if (x > bound && (x >> prev_s) == (bound >> prev_s)) cls[j] = 1;
                }
                n_app += cls[j] == 1 ? 1u : 0u;
            }
        }
        if (__any(n_app != 0)) {                                          // rare: fewer than SA_VTK_CAP entries in a whole call
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool keep = cls[j] == 1;
                const u64 b = __ballot(keep);
                u32 pos = 0;
                if (lane == 0 && b) pos = atomicAdd(&st->cand_cnt, (u32)__popcll(b));
                pos = (u32)__builtin_amdgcn_readfirstlane((int)pos) + (u32)__popcll(b & lt);
                if (keep && pos < SA_VTK_CAP) { cand_val[pos] = val[j]; cand_idx[pos] = idx[j]; }
            }
        }
        if (counting) {
            // Values cluster (a float64's first digit is its exponent, a constant vector has one digit at every level): the lanes that
            // share the first active lane's digit add once, together; the others add one by one.
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool mine = cls[j] == 2;
                const u64 act = __ballot(mine);
                if (act == 0) continue;                                   // (wave-uniform)
                const u32 d0 = (u32)__shfl((int)dg[j], (int)(__ffsll((long long)act) - 1), SA_WAVE);
                const u64 same = __ballot(mine && dg[j] == d0);
                if (lane == (u32)(__ffsll((long long)same) - 1)) atomicAdd(&h[d0], (u32)__popcll(same));
                if (mine && dg[j] != d0) atomicAdd(&h[dg[j]], 1u);
            }
        }
    }
    if (level == 0 && !have_bound && !take_all) {                         // the first pass counts the eligible entries (numFound)
        n_elig = sa_wave_sum(n_elig);
        if (lane == 0 && n_elig) atomicAdd(&st->found, (unsigned long long)n_elig);
    }
    if (counting) {
        __syncthreads();
        for (u32 i = tid; i < SA_VTK_BINS; i += SA_VTK_THREADS) {
            const u32 c = h[i];
            if (c) atomicAdd(&ghist[i], c);
        }
    }
}

// ---- find: the boundary bin of the level just counted ---------------------------------------------------------------------------
__global__ void __launch_bounds__(SA_VTK_THREADS) sa_k_vec_topk_find(sa_vtk_state* __restrict__ st, u32* __restrict__ ghist, u32 k, int tb) {
    __shared__ u32 red[SA_VTK_THREADS / SA_WAVE + 1];
    constexpr u32 PER = SA_VTK_BINS / SA_VTK_THREADS;                     // 16 bins a thread, highest bin first
    const u32 tid = threadIdx.x;
    const sa_vtk_state s = *st;
    __syncthreads();                                                      // (everyone has read the state before anyone writes it)
    if (s.done) return;
    if (s.append_bin || s.take_all) {                                     // the pass before this one was the last
        if (tid == 0) { st->done = 1; st->passes = s.passes + 1; }
        return;
    }
    const u32 k_rem = s.have_bound ? s.k_rem : k;
    u32 c[PER], sum = 0;
#pragma unroll
    for (u32 j = 0; j < PER; j++) {
        const u32 bin = SA_VTK_BINS - 1u - (tid * PER + j);
        c[j] = ghist[bin];
        ghist[bin] = 0;                                                   // ready for the next level
        sum += c[j];
    }
    u32 total = 0;
    const u32 above_me = sa_block_excl_scan<SA_VTK_THREADS / SA_WAVE>(sum, red, &total);
    if (!s.have_bound && total <= SA_VTK_CAP) {                           // few eligible entries (or fewer than k): sort them all
        if (tid == 0) { st->take_all = 1; st->passes = s.passes + 1; }
        return;
    }
    if (!(above_me < k_rem && k_rem <= above_me + sum)) return;           // exactly one thread owns the boundary bin
    u32 run = above_me, b = 0, binc = 0;
#pragma unroll
    for (u32 j = 0; j < PER; j++) {
        if (binc == 0 && run + c[j] >= k_rem) { b = SA_VTK_BINS - 1u - (tid * PER + j); binc = c[j]; }
        if (binc == 0) run += c[j];
    }
    const int p = sa_vtk_shift(tb, (int)s.level);
    const int fresh = s.have_bound ? (int)s.bound_p - p : SA_VTK_BITS;    // bits this digit adds below the old prefix
    const u128 old = ((u128)s.bound_hi << 64) | (u128)s.bound_lo;
    const u128 nb = s.have_bound ? ((old << fresh) | (u128)(b & ((1u << fresh) - 1u))) : (u128)b;
    st->bound_hi = (u64)(nb >> 64);
    st->bound_lo = (u64)nb;
    st->have_bound = 1;
    st->bound_p = (u32)p;
    st->prev_s = (u32)fresh;
    st->k_rem = k_rem - run;
    st->passes = s.passes + 1;
    // (entries above the boundary bins of all levels: fewer than k.  p == 0: the digit completes the key, the bin holds one entry)
    if (s.cand_cnt + run + binc <= SA_VTK_CAP) st->append_bin = 1;
    else st->level = s.level + 1;
}

// ---- final: sort the candidates, write the first k -------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) sa_k_vec_topk_final(const sa_vtk_state* __restrict__ st, const u64* __restrict__ cand_val,
                                                            const u64* __restrict__ cand_idx, u32 k, u64* __restrict__ out) {
    __shared__ u64 sv[SA_VTK_CAP];
    __shared__ u64 si[SA_VTK_CAP];
    if (!st->done) return;
    const u32 cnt = st->cand_cnt < SA_VTK_CAP ? st->cand_cnt : SA_VTK_CAP;
    u32 n2 = 2;
    while (n2 < cnt) n2 <<= 1;
    for (u32 i = threadIdx.x; i < n2; i += blockDim.x) {
        sv[i] = i < cnt ? cand_val[i] : 0ull;                             // padding ranks last: value 0, index 2^64-1
        si[i] = i < cnt ? cand_idx[i] : SA_NO_DOC;
    }
    for (u32 size = 2; size <= n2; size <<= 1) {
        for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (u32 t = threadIdx.x; t < (n2 >> 1); t += blockDim.x) {
                const u32 lo = 2 * t - (t & (stride - 1));
                const u32 hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const u64 xv = sv[lo], yv = sv[hi], xi = si[lo], yi = si[hi];
                const bool x_first = xv > yv || (xv == yv && xi < yi);    // value descending, then index ascending
                if (desc ? !x_first : x_first) { sv[lo] = yv; sv[hi] = xv; si[lo] = yi; si[hi] = xi; }
            }
        }
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < k; i += blockDim.x) {
        out[2 * i] = i < cnt ? sv[i] : 0ull;
        out[2 * i + 1] = i < cnt ? si[i] : SA_NO_DOC;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static int sa_vec_topk_scratch_get(sa_vec* v) {
    if (v->topk) return SA_OK;
    sa_vec_topk_scratch* s = new (std::nothrow) sa_vec_topk_scratch();
    if (!s) { sa_set_error("out of host memory"); return SA_ERR_NOMEM; }
    const size_t hist_b = SA_VTK_BINS * sizeof(u32), st_b = sizeof(sa_vtk_state), out_b = (size_t)SA_VTK_KMAX * 2 * sizeof(u64);
    const size_t cand_b = (size_t)SA_VTK_CAP * sizeof(u64);
    if (hipMalloc((void**)&s->d, hist_b + st_b + out_b + 2 * cand_b) != hipSuccess) {
        delete s;
        sa_set_error("hipMalloc failed (top-k scratch of a vector)");
        return SA_ERR_HIP;
    }
    s->hist = (u32*)s->d;
    s->st = (sa_vtk_state*)(s->d + hist_b);
    s->out = (u64*)(s->d + hist_b + st_b);
    s->cand_val = (u64*)(s->d + hist_b + st_b + out_b);
    s->cand_idx = (u64*)(s->d + hist_b + st_b + out_b + cand_b);
    s->host.resize((st_b + out_b) / sizeof(u64));
    v->topk = s;
    return SA_OK;
}

extern "C" int sa_vec_store(sa_vec_t* v, const void* host_in) {
    SA_ARG(v && (host_in || v->n == 0), "null argument");
    SA_HIP(hipSetDevice(v->device));
    hipStream_t st = sa_vec_stream(v->device);                            // (the vectors' stream, waited for: see sa_vec_create)
    if (v->n) SA_HIP(hipMemcpyAsync(v->d, host_in, (size_t)v->n * (v->f64 ? 8 : 4), hipMemcpyHostToDevice, st));
    SA_HIP(hipStreamSynchronize(st));
    return SA_OK;
}

extern "C" int sa_vec_topk(sa_vec_t* v, sa_filter_t* filter, int k, void* scores_out, uint64_t* docs_out, uint64_t* found_out) {
    SA_ARG(v && scores_out && docs_out, "null argument");
    SA_ARG(k >= 1 && k <= (int)SA_VTK_KMAX, "k must be in 1 .. SA_KMAX");
    SA_ARG(v->n < (1ull << 32), "vector too long (the histograms count in 32 bits)");
    const sa_filter_data* f = nullptr;
    if (filter) {
        SA_ARG(filter->d, "null filter");
        f = filter->d.get();
        SA_ARG(f->device == v->device, "the filter lives on another device than the vector");
        SA_ARG(f->n_docs == v->n, "the filter covers another number of documents than the vector holds");
    }
    const size_t vb = v->f64 ? 8 : 4;
    memset(scores_out, 0, (size_t)k * vb);
    for (int i = 0; i < k; i++) docs_out[i] = SA_NO_DOC;
    if (found_out) *found_out = 0;
    const u32 n_tiles = (u32)((v->n + SA_VTK_TILE - 1u) / SA_VTK_TILE);
    const u32 tile0 = f ? f->first_block : 0u;
    if (v->n == 0 || tile0 >= n_tiles) {                                  // nothing eligible: nothing is read
        if (v->topk) v->topk->passes = 0;
        return SA_OK;
    }
    SA_HIP(hipSetDevice(v->device));
    SA_TRY(sa_vec_topk_scratch_get(v));
    sa_vec_topk_scratch* s = v->topk;
    hipStream_t st = sa_vec_stream(v->device);
    int ib = 1;
    while ((1ull << ib) < v->n) ib++;
    const int tb = (v->f64 ? 63 : 31) + ib;
    const int n_levels = (tb + SA_VTK_BITS - 1) / SA_VTK_BITS;
    const u32 grid = n_tiles - tile0 < SA_VTK_MAX_GRID ? n_tiles - tile0 : SA_VTK_MAX_GRID;
    const u32* fwords = f ? (const u32*)f->d_words : nullptr;
    const u32* fblk = f ? (const u32*)f->d_blk : nullptr;
    SA_HIP(hipMemsetAsync(s->d, 0, SA_VTK_BINS * sizeof(u32) + sizeof(sa_vtk_state), st));
    const size_t back = sizeof(sa_vtk_state) + (size_t)k * 2 * sizeof(u64);
    const sa_vtk_state* hs = (const sa_vtk_state*)s->host.data();
    // The common case ends within three passes (two levels and the append); heavy ties take more rounds of one level each.
    int launched = 0;
    for (int round = 0; round <= n_levels + 1; round++) {
        const int passes = round == 0 ? 3 : 1;
        for (int i = 0; i < passes; i++, launched++) {
            if (v->f64) hipLaunchKernelGGL((sa_k_vec_topk_pass<true>), dim3(grid), dim3(SA_VTK_THREADS), 0, st, (const void*)v->d, v->n, fwords, fblk,
                                           tile0, n_tiles, ib, s->st, s->hist, s->cand_val, s->cand_idx);
            else hipLaunchKernelGGL((sa_k_vec_topk_pass<false>), dim3(grid), dim3(SA_VTK_THREADS), 0, st, (const void*)v->d, v->n, fwords, fblk,
                                    tile0, n_tiles, ib, s->st, s->hist, s->cand_val, s->cand_idx);
            hipLaunchKernelGGL(sa_k_vec_topk_find, dim3(1), dim3(SA_VTK_THREADS), 0, st, s->st, s->hist, (u32)k, tb);
        }
        hipLaunchKernelGGL(sa_k_vec_topk_final, dim3(1), dim3(1024), 0, st, (const sa_vtk_state*)s->st, (const u64*)s->cand_val,
                           (const u64*)s->cand_idx, (u32)k, s->out);
        SA_HIP(hipGetLastError());
        SA_HIP(hipMemcpyAsync(s->host.data(), s->st, back, hipMemcpyDeviceToHost, st));
        SA_HIP(hipStreamSynchronize(st));
        if (hs->done) break;
    }
    if (!hs->done) { sa_set_error("sa_vec_topk: the selection did not finish within %d passes", launched); return SA_ERR_STATE; }
    s->passes = (int)hs->passes;
    const u64* out = s->host.data() + sizeof(sa_vtk_state) / sizeof(u64);
    for (int i = 0; i < k; i++) {
        if (v->f64) ((u64*)scores_out)[i] = out[2 * i];
        else ((u32*)scores_out)[i] = (u32)out[2 * i];
        docs_out[i] = out[2 * i + 1];
    }
    if (found_out) *found_out = hs->found;
    return SA_OK;
}

// passes over the vector the last sa_vec_topk of `v` made (levels counted plus the appending pass): what DESIGN 3.6 quotes
extern "C" int sa_vec_topk_passes(const sa_vec_t* v, int* passes_out) {
    SA_ARG(v && passes_out, "null argument");
    *passes_out = v->topk ? v->topk->passes : 0;
    return SA_OK;
}
