// sa_bm25_params.hpp -- kernel parameter blocks shared by the BM25 scoring kernels (sa_bm25.hip: per-query and
// grouped tile kernels).
#pragma once
#include "sa_index.hpp"

struct alignas(16) sa_u64x2 { u64 x, y; };

// saturation table (sa_k_make_sattab, sa_bm25.hip): term frequencies 1 .. SA_SAT_NTF x doc lengths below at most SA_SAT_WMAX
#define SA_SAT_NTF 8
#define SA_SAT_WMAX 128
// grouped kernel (sa_k_bm25_group_tiles, sa_bm25.hip) and the grouping of a batch's rows (sa_batch.hip)
#define SA_GRP_MAXQ 16      // queries per table pass of a group item
#define SA_GRP_ITEM_ROUNDS 16    // items of 32 queries (two table passes) from this many rounds of 4096 one-pass items on; option group_item
#define SA_GRP_LOOSE_POSTINGS 400   // loose groups: expected postings of a query per tile, all terms together (SA_LOOSE_POSTINGS).  Round 3,
                                    // distinct-terms batch, 10 M docs: 64 / 96 / 128 / 192 / 256 / 384 / 512 -> 0.82 / 0.74 / 0.74 / 0.73 / 0.75 /
                                    // 0.80 / 0.81 ms at k = 10, hence 128.  Round 4, with the starting bounds (the per-query kernel AND the
                                    // overlay both start with a bound): 32 / 64 / 96 / 128 / 192 / 256 / 320 / 400 / 500 / 640 / 900 / all ->
                                    // 1.00 / 0.80 / 0.62 / 0.54 / 0.50 / 0.47 / 0.457 / 0.459 / 0.468 / 0.476 / 0.483 / 0.485 ms at k = 10;
                                    // k = 1000: 128 / 320 / 400 / 500 / 640 -> 0.89 / 0.84 / 0.81 / 0.77 / 0.81
// keys of one query the merge (sa_k_topk_merge) holds in LDS
#define SA_MERGE_LIST 2048

// Impact stream layout (sa_impacts, sa_index.hpp): first cell of term `term` whose TF postings start at tf_base
// (4 cells of slack per term: a term's last posting is followed by at least one whole, 16-byte-aligned pair
//  of sentinels before the next term starts -- the pair every load past a slice's term is clamped to)
__host__ __device__ __forceinline__ u64 sa_imp_base(u64 tf_base, u32 term) { return (tf_base + 4ull * term + 1ull) & ~1ull; }
// first cell of that sentinel pair, for a term of df postings starting at `ibase`
__host__ __device__ __forceinline__ u64 sa_imp_sentinel(u64 ibase, u64 df) { return ibase + ((df + 1ull) & ~1ull); }

struct Bm25Params {
    // index
    const u64* tfp;
    const u64* tf_off;
    const u32* dir_slot;
    const u32* tile_dir;
    const float* doc_lens;
    u32 n_terms, n_tiles;
    u64 n_docs, doc_base;
    int dl_packed;
    // batch
    const u32* terms;      // [B][T]
    const float* idf;      // [B][T]
    const float* sattab;   // [SA_SAT_NTF][tab_w] saturation table (sa_k_make_sattab)
    u32 tab_w;             // 0: no table (doc lengths not packed in the postings); else 64/128
    const u32* bounds;     // [B][T][n_tiles+1] slice table (sa_k_make_bounds)
    const u64* qbase;      // [B][T] posting base of each query term
    const u64* imp;        // impact stream (sa_impacts, sa_index.hpp) or null: score the TF postings
    const u64* qbase_imp;  // [B][T][2] impact stream: first cell of each query term, first cell of the sentinel pair behind it
    u64 imp_tail;          // a cell of the impact stream that is a sentinel whatever happens (its last pair)
    u32 B, T, k;
    u32 tile0, tile_end;   // tiles [tile0, tile_end) of this launch (sa_k_bm25_tiles)
    float k1, b, avgdl;
    int pruned;            // 1: wave-level selection against a global bound (MODE 1); 0: block-level selection (MODE 0)
    int no_topk;           // timing experiments only: skip the per-tile selection
    u32 cand_per_tile;     // general mode: candidate slots per (query, tile) = k
    u32 cand_cap;          // pruned mode: capacity of each query's append list
    u32* cand_cnt;         // pruned mode: [B] append cursors
    u32* slots;            // pruned mode: [B][32] pruning slots (score bits)
    u32* hist;             // pruned mode, k > 32: [B][SA_HBINS] score histograms (null: use the slots)
    u32* gthr;             // pruned mode, k > 32: [B] cached bound (score bits)
    const u32* seed;       // [B] the bound every query STARTS with (score bits; sa_k_make_bounds from the terms' rank tables), or null
    // dynamic pruning (MaxScore): per query the terms in ascending idf order and the score a doc
    // can reach at most from the j smallest-idf terms alone
    const float* ub;       // [B][T+1] upper bounds (ub[0] = 0), or null: exhaustive scoring
    const u32* ub_order;   // [B][T] query-term index of the j-th smallest idf
    const unsigned char* tf8;   // index dense tf rows [n_tf8_terms][n_docs]
    const u32* tf8_slot;   // [n_terms]
    u32* stats;            // diagnostics (sa_batch_stats): [B] candidates scored by the sparse path, or null
    const u32* qlist;      // queries to scan (after the sparse path took the others), or null: all B
    u32 nq;                // number of queries to scan (= B without a list)
    // occur classes (sa_batch_set_occur), or 0: u32[B][2] per device row -- the masks of the query's required and prohibited slots --
    // lie this many bytes behind `terms`, like the minimum-should-match values (min_match_off, which is then set as well and counts
    // the remaining, optional slots).  Only the occur instantiations of sa_k_bm25_tiles read them
    u32 occur_off;
    const u32* nq_dev;     // the same on the device (sa_k_bm25_tiles_list)
    // document filter of the batch (sa_filter.hpp), or null: every doc of the shard is eligible
    const u64* filt;       // one bit per local doc
    const u32* filt_blk;   // [filt_nblk] eligible docs per 1024-doc block
    u32 filt_nblk;
    // minimum-should-match (sa_batch_set_min_match), or 0: u32[B] per device row -- the number of query slots a doc must match to stay
    // in the ranking -- lie this many bytes behind `terms` (both are parts of the batch's upload block).  Only the counting
    // instantiations of sa_k_bm25_tiles read them (p.stats then counts the tiles they skipped)
    u32 min_match_off;
    // outputs
    float* dense_out;      // [B][n_docs] or null
    u64* cand;             // [B][n_tiles][k] composite keys (global doc ids) or null
};
// (min_match_off and occur_off sit in what was padding: the kernel arguments of every kernel stay where they were)
static_assert(sizeof(Bm25Params) == 336, "Bm25Params: a new field moves the kernel arguments of every BM25 kernel");

// host launchers of the BM25 kernels (sa_bm25.hip), called by the batch code (sa_batch.hip)
void sa_fill_params(const sa_index* ix, Bm25Params& p);
u32 sa_tile_waves(u32 tile_docs);
int sa_launch_bm25(sa_index* ix, const Bm25Params& p, hipStream_t st);                // per-query tile kernel (p.qlist: rows)
int sa_launch_bm25_list(sa_index* ix, const Bm25Params& p, hipStream_t st);           // ... over the device's query list
bool sa_min_match_tiles(u32 tile_docs);                                                // ... has counting instantiations (p.min_match_off, p.occur_off) for this tile size
int sa_launch_bm25_groups(sa_index* ix, const struct sa_batch* bt, const Bm25Params& p, u32 tile0, hipStream_t st);
