// sa_vec.hpp -- the handle of a dense per-doc device vector (Part 4 of the C ABI), shared by sa_vec.hip (create / combine / fetch) and
// sa_vec_topk.hip (store / top-k selection).
#pragma once
#include "sa_index.hpp"

struct sa_vec_topk_scratch;                      // sa_vec_topk.hip: histograms, candidate list, result staging

struct sa_vec {
    int device = 0;
    u64 n = 0;
    int f64 = 0;
    void* d = nullptr;
    sa_vec_topk_scratch* topk = nullptr;         // created by the first sa_vec_topk of this vector, freed by sa_vec_destroy
};

hipStream_t sa_vec_stream(int device);           // the stream of the vector kernels of `device` (sa_vec.hip)
void sa_vec_topk_release(sa_vec* v);             // frees v->topk (the vector's device is current)
