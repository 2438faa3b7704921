// sa_facet.hpp -- facet counts (Part 2d of the C ABI): a device column of category codes (sa_facet.hip) and the argument block of the
// counting kernels -- sa_k_bm25_facet_tiles (sa_bm25.hip, beside the tile item it calls) and sa_k_vec_facet (sa_facet.hip).
#pragma once
#include "sa_index.hpp"
#include "sa_bm25_params.hpp"

#define SA_FACET_LDS_BINS 1024u                  // columns of up to this many values are counted in an LDS histogram per workgroup
#define SA_FACET_MAX_VALUES (1u << 20)
#define SA_FACET_MAX_CELLS (1ull << 28)          // queries x values of one sa_batch_facet_counts call

// one int32 per (shard-local) document: -1 = no value, else a code in [0, n_values); checked at creation, immutable
struct sa_codes {
    int device = 0;
    u64 n_docs = 0;
    u32 n_values = 0;
    int* d = nullptr;
};

// What a counting kernel is handed beside Bm25Params (which is pinned at its size: sa_bm25_params.hpp), by value like GroupParams.
// The counters are u32, zeroed on the stream in front of the launch, and only ever touched by integer atomics.
struct FacetParams {
    const int* codes;       // [n_docs], or null: found only
    u32 n_values;
    u32* counts;            // [B][n_values] in CALLER query order
    u32* found;             // [B]
    u32* missing;           // [B]
    const u32* row;         // [B] device row -> caller query (sa_batch::d_perm)
};

// one workgroup per (tile, query) of p's tiles [tile0, tile_end) x rows [0, nq): sa_k_bm25_facet_tiles (sa_bm25.hip)
int sa_launch_bm25_facet(sa_index* ix, const Bm25Params& p, const FacetParams& fp, hipStream_t st);
