// sa_filter.hpp -- a document filter of one index (Part 2b of the C ABI, sa_filter.hip): an immutable bitmap over the shard-local
// documents that a BM25 batch (sa_batch_set_filter) or a phrase batch (sa_phrase_batch_set_filter) ranks inside.  Bit doc & 63 of word doc >> 6 (the same bytes read as u32
// words: bit doc & 31 of word doc >> 5); the bits from n_docs on are always 0, and the allocation runs one whole block past the
// last one, all zeros, so that a kernel may read the words of a whole tile of up to 1024 docs wherever the tile starts (kernels with
// larger tiles bound their reads by n_words).  blk[i] = eligible documents
// among [i * SA_FILTER_BLOCK, (i + 1) * SA_FILTER_BLOCK): every scoring tile size is a multiple of the block, so a tile kernel
// knows from its blocks' counts that a tile holds nothing without reading the words.
#pragma once
#include "sa_index.hpp"
#include <memory>

#define SA_FILTER_BLOCK 1024u                    // docs per summary cell (16 words)

struct sa_filter_data {
    const sa_index* ix = nullptr;                // the index it was built for (identity only: never dereferenced by a batch)
    int device = 0;
    u64 n_docs = 0, count = 0;                   // docs of the shard; eligible docs
    u64 n_words = 0;                             // u64 words that cover n_docs (the allocation holds n_alloc)
    u64 n_alloc = 0;
    u32 n_blocks = 0;
    u32 first_block = 0;                         // the first block with an eligible doc (n_blocks: none)
    u64* d_words = nullptr;
    u32* d_blk = nullptr;                        // [n_blocks + 1]
    ~sa_filter_data();
};

// the handle: batches share the data by reference count, so destroying the handle while a batch holds the filter is safe
struct sa_filter { std::shared_ptr<sa_filter_data> d; };
