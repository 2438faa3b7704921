"""sa_vec_store / sa_vec_topk (csrc/sa_vec_topk.hip): the k best entries of a dense device vector, optionally inside a DocFilter.

Every comparison is exact.  The yardstick is numpy on the host, written out in `yardstick` below: the entries with a value > 0
inside the mask, by value descending, then index ascending; padding is score 0 / row NO_DOC; `found` counts the eligible entries
whatever k is.  All cases run on the host-emulated kernels in the CPU suite and on the MI355X under -m gpu; the sizes only a GPU
can afford are marked gpu.  Added wall time of this file in the CPU suite: about 40 s."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from searcharray_amd import synth
from searcharray_amd._lib import SearchArrayHipError
from searcharray_amd.device_index import NO_DOC, DeviceIndex, DeviceVec

NS = [1, 63, 64, 65, 1023, 1025, 4097, 100_003]
KS = [1, 10, 32, 100, 1000, 1024]
DTYPES = [np.float32, np.float64]


def yardstick(v, mask, k):
    idx = np.flatnonzero((v > 0) & mask)
    order = np.lexsort((idx, -v[idx]))[:k]
    scores = np.zeros(k, dtype=v.dtype)
    rows = np.full(k, NO_DOC, dtype=np.uint64)
    scores[:len(order)] = v[idx[order]]
    rows[:len(order)] = idx[order]
    return scores, rows, len(idx)


def check(got, v, mask, k, what=""):
    want = yardstick(v, np.ones(len(v), bool) if mask is None else mask, k)
    assert got[0].dtype == v.dtype and got[1].dtype == np.uint64 and isinstance(got[2], int), what
    assert got[2] == want[2], f"{what}: found {got[2]} != {want[2]}"
    assert np.array_equal(got[1], want[1]), f"{what}: rows differ"
    assert np.array_equal(got[0], want[0]), f"{what}: scores differ"


def make_values(kind, n, dtype, seed=0):
    rng = np.random.default_rng([seed, n])
    if kind == "continuous":
        return (rng.random(n) * 20).astype(dtype)
    if kind == "quantised16":
        return ((rng.integers(0, 16, n) + 1) / 4).astype(dtype)
    if kind == "constant":
        return np.full(n, 2.5, dtype=dtype)
    if kind == "zeros":
        return np.zeros(n, dtype=dtype)
    if kind == "mixed":                                             # zeros, negatives and NaN never rank
        v = rng.standard_normal(n).astype(dtype)
        v[rng.random(n) < 0.2] = 0
        v[rng.random(n) < 0.1] = np.nan
        v[rng.random(n) < 0.05] = -0.0
        return v
    if kind == "below_f32":                                         # equal after rounding to float32, different in float64
        assert dtype == np.float64
        base = np.float64(np.float32(3.14159))
        v = base * (1 + rng.integers(-200, 200, n) * 2.0 ** -50)
        assert np.all(v.astype(np.float32) == np.float32(base)) and (n < 3 or len(np.unique(v)) > 1)
        return v
    if kind == "outlier_last":
        v = (rng.random(n) * 0.5).astype(dtype)
        v[-1] = 1e6
        return v
    raise AssertionError(kind)


KINDS = ["continuous", "quantised16", "constant", "zeros", "mixed", "below_f32", "outlier_last"]
VALUE_CASES = [(d, kind) for d in DTYPES for kind in KINDS if not (kind == "below_f32" and d == np.float32)]


def max_passes(n, f64):
    """the bound of the design: one pass per 12 bits of the key (63 or 31 value bits + the index bits) and the appending pass"""
    ib = max(1, int(n - 1).bit_length())
    return -(-((63 if f64 else 31) + ib) // 12) + 1


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dtype,kind", VALUE_CASES, ids=[f"{d.__name__}-{k}" for d, k in VALUE_CASES])
def test_topk_matches_numpy(api, on_emu, dtype, kind, n):
    v = make_values(kind, n, dtype)
    vec = DeviceVec(api, n, dtype == np.float64).store(v)
    try:
        ks = [10, 1024] if (on_emu and n > 5000) else KS          # (the emulator runs kernels on fibers: the largest n is thinned there)
        for k in ks:
            got = vec.topk(k)
            check(got, v, None, k, f"{kind} n={n} k={k}")
            assert vec.topk_passes() <= max_passes(n, dtype == np.float64)
            if kind == "constant":
                assert np.array_equal(got[1][:min(k, n)], np.arange(min(k, n), dtype=np.uint64))
            if kind == "zeros":
                assert got[2] == 0 and np.all(got[1] == NO_DOC) and np.all(got[0] == 0)
    finally:
        vec.close()


def small_index(api, n, seed=5):
    """an index of n documents: what a filter is built on (its postings do not matter here)"""
    lens, terms = synth.zipf_batch_tokens(0, n, 64, mean_len=2, seed=seed, fast=n > 200_000)
    words, counts = synth.encode_batch(lens, terms, 64)
    words, term_off = synth.concat_term_major([(words, counts)], 64)
    return DeviceIndex(words, term_off, lens.astype(np.float32), api=api)


def filter_masks(n, rng):
    full = np.ones(n, bool)
    empty = np.zeros(n, bool)
    tenth = rng.random(n) < 0.1
    span = np.zeros(n, bool)                                         # one range that starts past the first 1024-doc block
    lo = min(n - 1, 1024 + (n - 1024) // 3) if n > 1024 else n - 1
    span[lo:lo + max(1, (n - lo) // 2)] = True
    one = np.zeros(n, bool)
    one[(2 * n) // 3] = True
    return {"full": full, "empty": empty, "tenth": tenth, "span": span, "one": one}


@pytest.mark.parametrize("n", [1025, 4097, 100_003])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_topk_inside_a_filter(api, on_emu, dtype, n):
    rng = np.random.default_rng(n)
    ix = small_index(api, n)
    other = small_index(api, n, seed=6)                              # a filter of ANY index of that length will do
    vecs = {kind: (make_values(kind, n, dtype, seed=1), None) for kind in ("continuous", "quantised16", "constant")}
    try:
        for kind in vecs:
            vecs[kind] = (vecs[kind][0], DeviceVec(api, n, dtype == np.float64).store(vecs[kind][0]))
        for j, (name, mask) in enumerate(filter_masks(n, rng).items()):
            f = (other if j % 2 else ix).doc_filter(mask=mask)
            try:
                assert f.count() == int(mask.sum())
                for kind, (v, vec) in vecs.items():
                    for k in ([10] if (on_emu and n > 5000 and kind != "continuous") else [10, 1000]):
                        check(vec.topk(k, filter=f), v, mask, k, f"{kind} n={n} filter={name} k={k}")
                        assert (vec.topk_passes() == 0) == (name == "empty")     # an empty filter: nothing is read
            finally:
                f.close()
    finally:
        for _, vec in vecs.values():
            if vec is not None:
                vec.close()
        ix.close()
        other.close()


def test_filter_of_another_length_is_refused(api):
    ix = small_index(api, 1000)
    f = ix.doc_filter(mask=np.ones(1000, bool))
    vec = DeviceVec(api, 1001, True).store(np.ones(1001))
    try:
        with pytest.raises(SearchArrayHipError, match="another number of documents"):
            vec.topk(10, filter=f)
        for bad_k in (0, -1, 1025):
            with pytest.raises(ValueError):
                vec.topk(bad_k)
        with pytest.raises(SearchArrayHipError):                     # the C ABI checks k itself
            scores, rows = np.zeros(2000), np.zeros(2000, np.uint64)
            api.call("sa_vec_topk", vec._h, None, 1025, scores.ctypes.data, rows.ctypes.data_as(api.sa_vec_topk.argtypes[4]), None)
        with pytest.raises(ValueError):
            vec.store(np.ones(1000))
    finally:
        vec.close()
        f.close()
        ix.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_store_fetch_and_scratch_reuse(api, dtype):
    n = 30_011
    rng = np.random.default_rng(3)
    a, b = (rng.random(n) * 7).astype(dtype), ((rng.integers(0, 9, n)) / 3).astype(dtype)
    vec = DeviceVec(api, n, dtype == np.float64)
    try:
        assert np.array_equal(vec.fetch(), np.zeros(n, dtype))
        assert vec.topk_passes() == 0
        check(vec.topk(5), np.zeros(n, dtype), None, 5, "fresh vector")
        vec.store(a)
        assert np.array_equal(vec.fetch(), a)
        check(vec.topk(100), a, None, 100, "first")
        check(vec.topk(100), a, None, 100, "second call, same scratch")
        check(vec.topk(7), a, None, 7, "other k")
        vec.store(b)                                                 # overwritten: the new answer, nothing kept from the old one
        assert np.array_equal(vec.fetch(), b)
        check(vec.topk(100), b, None, 100, "after overwrite")
        vec.zero()
        check(vec.topk(100), np.zeros(n, dtype), None, 100, "after zero")
    finally:
        vec.close()


def test_eight_threads_each_with_its_own_vector(api):
    n = 20_001
    rng = np.random.default_rng(8)
    data = [(rng.random(n) * 3).astype(np.float64 if i % 2 else np.float32) for i in range(8)]
    data[3] = np.round(data[3], 1)                                   # heavy ties in one of them
    serial = []
    for v in data:
        vec = DeviceVec(api, n, v.dtype == np.float64).store(v)
        serial.append(vec.topk(50))
        vec.close()
        check(serial[-1], v, None, 50, "serial")

    def work(i):
        vec = DeviceVec(api, n, data[i].dtype == np.float64).store(data[i])
        try:
            return [vec.topk(50) for _ in range(3)]
        finally:
            vec.close()

    with ThreadPoolExecutor(max_workers=8) as ex:
        for i, results in enumerate(ex.map(work, range(8))):
            for got in results:
                assert got[2] == serial[i][2] and np.array_equal(got[0], serial[i][0]) and np.array_equal(got[1], serial[i][1]), i


@pytest.mark.parametrize("k", [10, 1000])
def test_300k_float64(api, k):
    n = 300_000
    v = np.random.default_rng(30).gamma(2.0, 3.0, n)
    v[::7] = 0
    vec = DeviceVec(api, n, True).store(v)
    try:
        check(vec.topk(k), v, None, k, f"300k k={k}")
        assert vec.topk_passes() <= max_passes(n, True)
    finally:
        vec.close()


# ---- sizes for the GPU only -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_api():
    from searcharray_amd import _lib
    return _lib.api()


@pytest.fixture(scope="module")
def index_2m(gpu_api):
    ix = small_index(gpu_api, 2_000_000)
    yield ix
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True], ids=["all", "tenth"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_2m_entries(gpu_api, index_2m, dtype, filtered):
    n = 2_000_000
    rng = np.random.default_rng(2)
    v = rng.gamma(2.0, 3.0, n).astype(dtype)
    v[rng.random(n) < 0.3] = 0
    mask = rng.random(n) < 0.1 if filtered else None
    f = index_2m.doc_filter(mask=mask) if filtered else None
    vec = DeviceVec(gpu_api, n, dtype == np.float64).store(v)
    try:
        for k in (10, 1000):
            check(vec.topk(k, filter=f), v, mask, k, f"2M {dtype.__name__} filtered={filtered} k={k}")
            assert vec.topk_passes() <= max_passes(n, dtype == np.float64)
    finally:
        vec.close()
        if f is not None:
            f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: d.__name__)
def test_10m_entries(gpu_api, dtype):
    n = 10_000_000
    v = np.random.default_rng(10).gamma(2.0, 3.0, n).astype(dtype)
    vec = DeviceVec(gpu_api, n, dtype == np.float64).store(v)
    try:
        for k in (10, 1000):
            check(vec.topk(k), v, None, k, f"10M {dtype.__name__} k={k}")
    finally:
        vec.close()


@pytest.mark.gpu
def test_10m_constant_vector_takes_the_worst_case_pass_count(gpu_api):
    """every value ties: the selection refines through all the value bits and then the index bits, one level a pass.  The key has
    63 + 24 = 87 bits = 8 levels; seven are counted (after the seventh a boundary bin holds the 8 entries that share all but the
    last 3 index bits, which fits the candidate list, so the eighth level is not needed) and one pass appends: 8 passes, one below
    the bound of 9 that holds for any data"""
    n = 10_000_000
    v = np.full(n, 1.75)
    vec = DeviceVec(gpu_api, n, True).store(v)
    try:
        got = vec.topk(1000)
        check(got, v, None, 1000, "10M constant")
        assert np.array_equal(got[1], np.arange(1000, dtype=np.uint64))
        assert max_passes(n, True) == 9 and vec.topk_passes() == 8
    finally:
        vec.close()
