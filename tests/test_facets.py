"""Hit counts and facet counts, counted on the device (Part 2d: sa_codes_*, sa_batch_facet_counts, sa_vec_facet_counts;
QueryBatch.facet_counts, DeviceVec.facet_counts, SearchArray.facets / count, solr.edismax_facets).

The expectation, for every case, comes from the oracle's dense vector `d` of the query -- the formula of tests/test_occur.py
(`dense_of`: the slots' scores summed in slot order, cleared where the occur classes / the minimum-should-match value say so), then
the document mask -- and numpy:

    found   = (d > 0).sum()
    missing = ((d > 0) & (codes < 0)).sum()
    counts  = np.bincount(codes[(d > 0) & (codes >= 0)], minlength=V)

Every comparison is np.array_equal.  The module asserts from the oracle alone that the cases cannot pass vacuously (section 9)."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from searcharray_amd import _lib, synth
from searcharray_amd import roaringish as rz
from searcharray_amd._lib import SearchArrayHipError
from searcharray_amd.device_index import DeviceIndex, DeviceVec, FacetColumn, FacetCounts
from searcharray_amd.postings import SearchArray
from searcharray_amd.solr import edismax, edismax_facets, edismax_search
from tests.test_abi import declared_functions
from tests.test_filter import the_masks
from tests.test_min_match import band, head_queries
from tests.test_min_match import corpus  # noqa: F401  (the module's fixture: synth.corpus_triples(9000, 400, 14, seed=31))
from tests.test_occur import dense_of, pattern

N_DOCS, VOCAB = 9000, 400
NO_DOC = np.uint64(2**64 - 1)
UNSUPPORTED = r"\(-5\)"                                       # SA_ERR_UNSUPPORTED in the error text
BAD_ARG = r"\(-2\)"                                           # SA_ERR_ARG
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edismax.npz")
TILES = [1024, 2048, 4096, 8192]
MODES = ("plain", "m2", "mT", "must0", "not0", "mix_m")


# ---- the columns (all random parts from default_rng(7), in this order)
def the_columns():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 7, N_DOCS).astype(np.int32)
    a[rng.random(N_DOCS) < 0.1] = -1                          # (a) V = 7, uniform, 10 % without a value: the LDS histogram
    b = rng.integers(0, 3000, N_DOCS).astype(np.int32)        # (b) V = 3000: the direct atomics
    c = (np.arange(N_DOCS) // 1500).astype(np.int32)          # (c) V = 6: whole waves hit one bin
    d1024 = rng.integers(0, 1024, N_DOCS).astype(np.int32)    # (d) the two sides of the path switch
    d1025 = rng.integers(0, 1025, N_DOCS).astype(np.int32)
    d1025[:3] = 1024                                          # (the last bin of the larger column is in use)
    e = np.full(N_DOCS, -1, dtype=np.int32)                   # (e) no doc has a value
    return {"a": (a, 7), "b": (b, 3000), "c": (c, 6), "d1024": (d1024, 1024), "d1025": (d1025, 1025), "e": (e, 4)}


def the_filters():
    """a random 10 % mask, a contiguous 1 % range, the empty filter"""
    rng = np.random.default_rng(7)
    m10 = rng.random(N_DOCS) < 0.10
    rg = np.zeros(N_DOCS, dtype=bool)
    rg[4000:4090] = True
    return {"10%": m10, "range": rg, "empty": np.zeros(N_DOCS, dtype=bool)}


def mode_of(mode, T):
    """(occur classes of the T slots, m) of a mode"""
    if mode == "plain":
        return [0] * T, 0
    if mode == "m2":
        return [0] * T, 2
    if mode == "mT":
        return [0] * T, T
    return pattern(mode, T)


# the oracle's dense vectors, computed once per (query, classes, m) and shared by every test of the module (never modified)
_dense = {}


def dense(orc, q, occ, m):
    key = (np.asarray(q).tobytes(), tuple(int(x) for x in occ), int(m))
    if key not in _dense:
        d = dense_of(orc, q, occ, int(m))
        d.setflags(write=False)
        _dense[key] = d
    return _dense[key]


def want_one(d, codes, V, mask=None):
    hit = d > 0
    if mask is not None:
        hit = hit & mask
    return int(hit.sum()), int((hit & (codes < 0)).sum()), np.bincount(codes[hit & (codes >= 0)], minlength=V)


def want_all(orc, queries, occs, ms, codes, V, mask=None):
    rows = [want_one(dense(orc, q, occ, m), codes, V, mask) for q, occ, m in zip(queries, occs, ms)]
    return (np.asarray([r[0] for r in rows], dtype=np.int64), np.asarray([r[1] for r in rows], dtype=np.int64),
            np.stack([r[2] for r in rows]).astype(np.int64))


def check(got, want, what):
    found, missing, counts = got
    assert found.dtype == np.int64 and missing.dtype == np.int64 and counts.dtype == np.int64, what
    assert np.array_equal(found, want[0]), f"{what}: found {found[:6]} != {want[0][:6]}"
    assert np.array_equal(missing, want[1]), f"{what}: missing"
    assert counts.shape == want[2].shape and np.array_equal(counts, want[2]), f"{what}: counts"
    assert np.array_equal(counts.sum(1) + missing, found), f"{what}: counts + missing != found"


def set_mode(bt, mode, T, n):
    occ, m = mode_of(mode, T)
    bt.set_occur(None if not any(occ) else np.tile(np.asarray(occ, dtype=np.uint8), (n, 1)))
    bt.set_min_match(None if m == 0 else [m] * n)
    return [occ] * n, [m] * n


def query_sets():
    return {"head": (head_queries(4), 4), "band": (band(8), 8)}


# ---- 9. not vacuous, from the oracle alone (called by the first test of section 1 before any device call)
def assert_not_vacuous(orc):
    codes, V = the_columns()["a"]
    mask = the_filters()["10%"]
    queries = head_queries(4)
    assert len(queries) == 40
    plain = [want_one(dense(orc, q, [0] * 4, 0), codes, V) for q in queries]
    assert sum(p[0] > 50 for p in plain) >= 30, "found > 50: nothing here can be derived from a top-k"
    vectors = {tuple(p[2]) for p in plain}
    assert len(vectors) >= 30, f"only {len(vectors)} distinct count vectors"
    full = [want_one(dense(orc, q, [0] * 4, 4), codes, V) for q in queries]
    assert sum(not np.array_equal(p[2], f[2]) for p, f in zip(plain, full)) >= 30, "m = T changes the counts"
    masked = [want_one(dense(orc, q, [0] * 4, 0), codes, V, mask) for q in queries]
    assert sum(not np.array_equal(p[2], f[2]) for p, f in zip(plain, masked)) >= 30, "the 10 % mask changes the counts"
    assert sum(f[0] > 0 for f in full) >= 30 and sum(f[0] > 0 for f in masked) >= 30, "the restricted cases still have hits"
    # every mode leaves most queries of its set hits
    for name, (qs, T) in query_sets().items():
        for mode in MODES:
            occ, m = mode_of(mode, T)
            hits = sum(bool((dense(orc, q, occ, m) > 0).any()) for q in qs)
            if not (name == "band" and mode == "mT"):            # (no doc holds all eight terms of a band query: the zeros case)
                assert hits >= 20, f"{name} {mode}: {hits} of 40 queries with a hit"


# ---- 1. tile sizes x modes x columns x query sets
def cells():
    return [(qs, mode, col) for qs in ("head", "band") for mode in MODES for col in ("a", "b", "c")]


def cells_for(on_emu, tile):
    """all 36 cells on the GPU; the host-emulated kernels take every third per tile size, shifted with it -- (query set, mode) pairs
    are 3 cells apart, so each tile size sees every pair once, with a column that rotates -- plus one cell of every column"""
    all_cells = cells()
    if not on_emu:
        return all_cells
    shift = TILES.index(tile)
    picked = [c for i, c in enumerate(all_cells) if (i + i // 3) % 3 == shift % 3]
    return picked


def test_the_emulator_subsets_cover_every_cell_kind():
    for tile in TILES:
        picked = cells_for(True, tile)
        assert {(c[0], c[1]) for c in picked} == {(c[0], c[1]) for c in cells()}, "every (query set, mode) at every tile size"
        assert {c[2] for c in picked} == {"a", "b", "c"}
    assert {c for tile in TILES[:3] for c in cells_for(True, tile)} == set(cells()), "every cell on some tile size"


@pytest.mark.parametrize("tile", TILES)
def test_every_tile_size_mode_and_column(api, corpus, on_emu, tile):
    words, off, lens, orc = corpus
    if tile == TILES[0]:
        assert_not_vacuous(orc)
    cols = the_columns()
    dev = DeviceIndex(words, off, lens, tile_docs=tile, api=api)
    dcol = {name: dev.facet_column(*cols[name]) for name in ("a", "b", "c")}
    batches = {name: dev.batch(qs, k=10) for name, (qs, T) in query_sets().items()}
    for qs_name, mode, col in cells_for(on_emu, tile):
        queries, T = query_sets()[qs_name]
        bt = batches[qs_name]
        occs, ms = set_mode(bt, mode, T, len(queries))
        what = f"tile {tile} {qs_name} {mode} column {col}"
        check(bt.facet_counts(dcol[col]), want_all(orc, queries, occs, ms, *cols[col]), what)
    # found alone (codes == NULL), in the state the last cell left
    found, missing, counts = bt.facet_counts()
    assert counts is None and not missing.any()
    assert np.array_equal(found, want_all(orc, queries, occs, ms, *cols["a"])[0]), f"tile {tile}: found alone"
    for x in list(batches.values()) + list(dcol.values()):
        x.close()
    dev.close()


def test_the_path_switch_and_a_column_without_values(api, corpus):
    """(d) V = 1024 (the LDS histogram's last size) and V = 1025 (the first with direct atomics) on one query set; (e) all -1"""
    words, off, lens, orc = corpus
    cols = the_columns()
    dev = DeviceIndex(words, off, lens, tile_docs=2048, api=api)
    queries = head_queries(4)
    bt = dev.batch(queries, k=10)
    occs, ms = [[0] * 4] * 40, [0] * 40
    for name in ("d1024", "d1025", "e"):
        col = dev.facet_column(*cols[name])
        assert isinstance(col, FacetColumn) and col.n_values == cols[name][1]
        got = bt.facet_counts(col)
        check(got, want_all(orc, queries, occs, ms, *cols[name]), name)
        if name == "d1025":
            assert got[2][:, 1024].sum() >= 1, "the last bin of the larger column counts"
        if name == "e":
            assert not got[2].any() and np.array_equal(got[1], got[0]) and got[0].all()
        col.close()
    bt.close()
    dev.close()


# ---- 2. with a filter
@pytest.mark.parametrize("tile", [1024, 4096])
def test_with_a_filter(api, corpus, tile):
    words, off, lens, orc = corpus
    cols = the_columns()
    dev = DeviceIndex(words, off, lens, tile_docs=tile, api=api)
    queries = head_queries(4)
    bt = dev.batch(queries, k=10)
    ca, cb = dev.facet_column(*cols["a"]), dev.facet_column(*cols["b"])
    occs = [[0] * 4] * 40
    for name, mask in the_filters().items():
        f = dev.doc_filter(mask=mask)
        bt.set_filter(f)
        for m in (0, 2):
            bt.set_min_match(None if m == 0 else [m] * 40)
            for cname, col in (("a", ca), ("b", cb)):
                got = bt.facet_counts(col)
                check(got, want_all(orc, queries, occs, [m] * 40, *cols[cname], mask=mask), f"tile {tile} filter {name} m {m} column {cname}")
                if name == "empty":
                    assert not got[0].any() and not got[2].any()
        f.close()
    # a filter of the module next door, and the filter cleared again
    m5 = the_masks()["5%"]
    f = dev.doc_filter(mask=m5)
    bt.set_filter(f)
    bt.set_min_match(None)
    check(bt.facet_counts(ca), want_all(orc, queries, occs, [0] * 40, *cols["a"], mask=m5), "5% mask")
    bt.set_filter(None)
    check(bt.facet_counts(ca), want_all(orc, queries, occs, [0] * 40, *cols["a"]), "filter cleared")
    for x in (f, ca, cb, bt, dev):
        x.close()


# ---- 3. a reordered batch with per-query values
def test_a_reordered_batch_reports_in_caller_order(api, corpus):
    words, off, lens, orc = corpus
    cols = the_columns()
    dev = DeviceIndex(words, off, lens, tile_docs=2048, api=api)
    rng = np.random.default_rng(17)
    queries = np.stack([rng.choice(16, 4, replace=False) for _ in range(200)])
    ms = rng.integers(0, 6, 200)
    assert len(set(ms)) == 6
    bt = dev.batch(queries, k=20, min_match=ms)
    rows = bt.row_order()
    assert sorted(rows) == list(range(200)) and not np.array_equal(rows, np.arange(200)), "the device rows are not in caller order"
    for name in ("a", "b"):
        col = dev.facet_column(*cols[name])
        got = bt.facet_counts(col)
        check(got, want_all(orc, queries, [[0] * 4] * 200, ms, *cols[name]), f"reordered, column {name}")
        assert not got[0][ms == 5].any() and got[0][ms == 4].any() and len(set(got[0])) > 50
        col.close()
    bt.close()
    dev.close()


# ---- 4. doc_base != 0: the codes are indexed by local row
def test_doc_base(api, corpus):
    words, off, lens, orc = corpus
    cols = the_columns()
    dev = DeviceIndex(words, off, lens, tile_docs=1024, doc_base=50_000, api=api)
    queries = band(8)
    bt = dev.batch(queries, k=10, min_match=[2] * 40)
    for name in ("a", "b"):
        col = dev.facet_column(*cols[name])
        check(bt.facet_counts(col), want_all(orc, queries, [[0] * 8] * 40, [2] * 40, *cols[name]), f"doc_base, column {name}")
        col.close()
    bt.close()
    dev.close()


# ---- 5. an unfetched run is left intact; counts follow the batch's state
def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("route", ["staged", "pruned"])
def test_an_unfetched_run_is_left_intact(api, corpus, route):
    words, off, lens, orc = corpus
    cols = the_columns()
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    queries, other = band(8), band(8)[::-1].copy()
    bt = dev.batch(queries, k=10)
    if route == "pruned":
        bt.set_options(stage=0, sparse=1)
        bt.reset(queries)
    ca, cb = dev.facet_column(*cols["a"]), dev.facet_column(*cols["b"])
    bt.run()
    assert bt.last_route() == route
    ref = bt.fetch()
    assert (ref[0] > 0).any()
    occs = [[0] * 8] * 40
    for col, name in ((ca, "a"), (cb, "b"), (None, "none")):
        bt.run(sync=False)
        got = bt.facet_counts(col)
        assert same(bt.fetch(), ref), f"{route}: the run in flight when column {name} was counted"
        if col is not None:
            check(got, want_all(orc, queries, occs, [0] * 40, *cols[name]), f"{route} column {name}")
    bt.run()
    assert same(bt.fetch(), ref) and bt.last_route() == route, "the next run"
    # counts follow reset / step, and the filter state
    bt.reset(other)
    check(bt.facet_counts(ca), want_all(orc, other, occs, [0] * 40, *cols["a"]), f"{route}: after reset")
    idf = np.asarray([dev.idfs([t])[0] for t in range(VOCAB)], dtype=np.float32)
    dev.set_idf_table(idf)
    bt.step(queries)
    got = bt.facet_counts(ca)
    stepped = bt.fetch()
    check(got, want_all(orc, queries, occs, [0] * 40, *cols["a"]), f"{route}: after step")
    assert same(stepped, ref), "the step's run, counted before it was fetched"
    mask = the_filters()["10%"]
    f = dev.doc_filter(mask=mask)
    bt.set_filter(f)
    check(bt.facet_counts(ca), want_all(orc, queries, occs, [0] * 40, *cols["a"], mask=mask), f"{route}: filter set")
    bt.set_filter(None)
    check(bt.facet_counts(ca), want_all(orc, queries, occs, [0] * 40, *cols["a"]), f"{route}: filter cleared")
    bt.run()
    assert same(bt.fetch(), ref)
    for x in (f, ca, cb, bt, dev):
        x.close()


# ---- 6. invariants against search itself
def test_found_is_what_search_returns(api, corpus):
    """band queries whose matches fit k = 1000: found equals the used slots of the ranking, and the facet of the ranked rows' codes
    equals the counts"""
    words, off, lens, orc = corpus
    codes, V = the_columns()["a"]
    dev = DeviceIndex(words, off, lens, tile_docs=2048, api=api)
    col = dev.facet_column(codes, V)
    queries = band(8)
    small = 0
    for m in (0, 2):
        bt = dev.batch(queries, k=1000, min_match=[m] * 40)
        bt.run()
        scores, docs = bt.fetch()
        found, missing, counts = bt.facet_counts(col)
        assert np.array_equal(counts.sum(1) + missing, found)
        for qi in range(40):
            used = int((scores[qi] > 0).sum())
            if found[qi] <= 1000:
                small += 1
                assert used == found[qi], f"m {m} q{qi}: {used} used slots, found {found[qi]}"
                rows = docs[qi, :used].astype(np.int64)
                assert np.array_equal(np.bincount(codes[rows][codes[rows] >= 0], minlength=V), counts[qi]), f"m {m} q{qi}"
                assert int((codes[rows] < 0).sum()) == missing[qi]
            else:
                assert used == 1000
        bt.close()
    assert small >= 30, f"only {small} of 80 rankings fit k = 1000"
    col.close()
    dev.close()


# ---- 7. device vectors and edismax
@pytest.mark.parametrize("f64", [False, True])
def test_vec_facet_counts(api, corpus, f64):
    words, off, lens, orc = corpus
    cols = the_columns()
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    rng = np.random.default_rng(7)
    dt = np.float64 if f64 else np.float32
    x = rng.random(N_DOCS).astype(dt)
    x[rng.random(N_DOCS) < 0.3] = 0
    x[rng.random(N_DOCS) < 0.1] *= -1
    x[::97] = np.nan
    x[5::501] = np.inf
    assert np.isnan(x).sum() > 50 and (x < 0).sum() > 100 and (x == 0).sum() > 1000 and (x > 0).sum() > 3000
    v = DeviceVec(api, N_DOCS, f64).store(x)
    hit = x > 0
    filters = dict(the_filters(), none=None)
    for name in ("a", "b", "d1024", "d1025", "e"):
        codes, V = cols[name]
        col = dev.facet_column(codes, V)
        for fname, mask in filters.items():
            f = None if mask is None else dev.doc_filter(mask=mask)
            found, missing, counts = v.facet_counts(col, filter=f)
            h = hit if mask is None else hit & mask
            assert isinstance(found, int) and isinstance(missing, int) and counts.dtype == np.int64
            assert found == int(h.sum()) and missing == int((h & (codes < 0)).sum()), f"{name} {fname}"
            assert np.array_equal(counts, np.bincount(codes[h & (codes >= 0)], minlength=V)), f"{name} {fname}"
            assert v.facet_counts(None, filter=f) == (found, 0, None)
            assert v.topk(1, filter=f)[2] == found, "the eligibility is sa_vec_topk's"
            if f is not None:
                f.close()
        col.close()
    v.close()
    dev.close()
    # five entries
    t5 = synth.corpus_triples(5, 10, 3, seed=1)
    w5, wt5 = rz.encode_sorted(t5[0], t5[1], t5[2])
    d5 = DeviceIndex(w5, rz.term_offsets(wt5, 10), t5[3], api=api)
    c5 = np.asarray([0, 1, -1, 1, 2], dtype=np.int32)
    col = d5.facet_column(c5, 3)
    for vals in ([1.0, np.nan, 2.0, -1.0, 0.5], [0.0, 0.0, 0.0, 0.0, 0.0], [np.inf, 3.0, 1e-30, 2.0, 7.0]):
        v = DeviceVec(api, 5, f64).store(vals)
        h = np.asarray(vals, dtype=dt) > 0
        for mask in (None, np.asarray([1, 1, 0, 0, 1], dtype=bool), np.zeros(5, dtype=bool)):
            f = None if mask is None else d5.doc_filter(mask=mask)
            hh = h if mask is None else h & mask
            found, missing, counts = v.facet_counts(col, filter=f)
            assert (found, missing) == (int(hh.sum()), int((hh & (c5 < 0)).sum())), (vals, mask)
            assert np.array_equal(counts, np.bincount(c5[hh & (c5 >= 0)], minlength=3)), (vals, mask)
        v.close()
    # a column or a filter of another length
    v = DeviceVec(api, 6, f64)
    with pytest.raises(SearchArrayHipError, match=BAD_ARG):
        v.facet_counts(col)
    with pytest.raises(TypeError):
        v.facet_counts(c5)
    v.close()
    col.close()
    d5.close()


def _lower_whole(text):
    return [text.lower()]


@pytest.fixture(scope="module")
def golden(default_api):
    g = np.load(GOLDEN, allow_pickle=False)
    frame = pd.DataFrame({"title": SearchArray.index(list(g["field_title"])),
                          "body": SearchArray.index(list(g["field_body"])),
                          "tags": SearchArray.index(list(g["field_tags"]), tokenizer=_lower_whole)})
    return g, frame, json.loads(str(g["cases"]))


def test_edismax_facets(golden):
    g, frame, cases = golden
    n = len(frame)
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 5, n).astype(np.int64)
    codes[rng.random(n) < 0.1] = -1
    brand = pd.Series(pd.Categorical.from_codes(codes, categories=["acme", "bolt", "core", "dyna", "echo"]))
    mask = rng.random(n) < 0.4
    title = frame["title"].array
    col = title.facet_column(brand)
    assert list(col.categories) == ["acme", "bolt", "core", "dyna", "echo"] and col.n_values == 5
    with_pf = [i for i, c in enumerate(cases) if c.get("pf") or c.get("pf2") or c.get("pf3")]
    assert with_pf, "the goldens hold cases with phrase boosts"
    dtypes = set()
    for case in sorted(set([0, 3, 7, 11] + with_pf[:2])):
        params = {k: v for k, v in cases[case].items() if k in ("q", "qf", "mm", "pf", "pf2", "pf3", "tie", "q_op")}
        assert len(params) == len(cases[case]), cases[case]
        scores, _ = edismax(frame, **params)
        dtypes.add(scores.dtype)
        for fq, m in ((None, np.ones(n, dtype=bool)), (mask, mask), (np.flatnonzero(mask)[::-1], mask), (title.doc_filter(mask), mask)):
            hit = (scores > 0) & m
            want = np.bincount(codes[hit & (codes >= 0)], minlength=5)
            for by in (col, brand, brand.array, codes):
                for route in (True, False):
                    if not route and (by is col or not (fq is None or isinstance(fq, np.ndarray))):
                        continue                                      # (the host route takes host codes and host filters)
                    got = edismax_facets(frame, by=by, fq=fq, use_device=route, **params)
                    what = f"case {case} route {route}"
                    assert isinstance(got, FacetCounts) and got.found == int(hit.sum()), what
                    assert got.missing == int((hit & (codes < 0)).sum()) and np.array_equal(got.counts, want), what
                    assert got.counts.dtype == np.int64 and int(got.counts.sum()) + got.missing == got.found
                    assert (got.categories is None) == (by is codes), what
            assert edismax_facets(frame, by=col, fq=fq, **params).found == edismax_search(frame, fq=fq, **params).found
        assert int(((scores > 0) & mask).sum()) not in (0, int((scores > 0).sum())), "the fq changes the hit count"
    assert dtypes == {np.dtype(np.float32), np.dtype(np.float64)}, "term-centric and field-centric cases"
    col.close()
    with pytest.raises(ValueError):
        edismax_facets(frame, by=codes[:-1], **params)


# ---- 8. SearchArray.facets / count
def test_search_array_facets_and_count(default_api):
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(30)]
    p = 1.0 / np.arange(1, 31)
    p /= p.sum()
    docs = [" ".join(rng.choice(vocab, size=max(1, rng.poisson(12)), p=p)) for _ in range(700)]
    arr = SearchArray.index(docs)
    n = len(arr)
    codes = np.random.default_rng(7).integers(-1, 4, n)
    colour = pd.Series(pd.Categorical.from_codes(codes, categories=["red", "green", "blue", "grey"]))
    strings = ["w0 w7 w20", "w3 w29 w1 w2", "w1", "nope w2 w0", "w5 w5 w11", "w0 w1 w2 w3 w4"]
    K = 700

    def want(**kw):
        scores, ids = arr.search(strings, k=K, **kw)
        rows = [ids[i][scores[i] > 0].astype(np.int64) for i in range(len(strings))]
        return (np.asarray([len(r) for r in rows]), np.asarray([int((codes[r] < 0).sum()) for r in rows]),
                np.stack([np.bincount(codes[r][codes[r] >= 0], minlength=4) for r in rows]))

    col = arr.facet_column(colour)
    assert isinstance(col, FacetColumn) and col.n_values == 4 and list(col.categories) == ["red", "green", "blue", "grey"]
    mask = np.random.default_rng(4).random(n) < 0.5
    prefixed = ["+w0 w7 -w20", "-w3 w29 +w1 w2", "w1", "-nope +w2 w0", "+w5 w5 -w11", "w0 +w1 -w2 w3 w4"]
    seen = []
    for kw, qs in (({}, strings), ({"mm": 2}, strings), ({"q_op": "AND"}, strings), ({"filter": mask}, strings),
                   ({"filter": np.flatnonzero(mask), "mm": "2"}, strings), ({"filter": arr.doc_filter(mask)}, strings),
                   ({"occur": "prefix"}, prefixed), ({"occur": "prefix", "mm": 1, "filter": mask}, prefixed)):
        w = want(**kw) if qs is strings else None
        if w is None:
            scores, ids = arr.search(qs, k=K, **kw)
            rows = [ids[i][scores[i] > 0].astype(np.int64) for i in range(len(qs))]
            w = (np.asarray([len(r) for r in rows]), np.asarray([int((codes[r] < 0).sum()) for r in rows]),
                 np.stack([np.bincount(codes[r][codes[r] >= 0], minlength=4) for r in rows]))
        for by in (col, colour, codes):
            got = arr.facets(qs, by, **kw)
            assert isinstance(got, FacetCounts), kw
            check((got.found, got.missing, got.counts), w, f"facets {kw}")
            assert (got.categories is None) == (by is codes)
            if got.categories is not None:
                assert list(got.categories) == ["red", "green", "blue", "grey"]
        cnt = arr.count(qs, **kw)
        assert cnt.dtype == np.int64 and np.array_equal(cnt, w[0]), f"count {kw}"
        seen.append(tuple(w[0]))
    assert len(set(seen)) >= 6, "the arguments change the counts"
    # q_op = AND with an unknown token: zeros for that query
    got = arr.facets(strings, col, q_op="AND")
    assert got.found[3] == 0 and not got.counts[3].any() and got.found[0] > 0
    # B = 0
    got = arr.facets([], col)
    assert got.found.shape == (0,) and got.missing.shape == (0,) and got.counts.shape == (0, 4) and arr.count([]).shape == (0,)
    # n_values: defaults to max + 1, may be larger
    c2 = arr.facet_column(np.maximum(codes, 0))
    assert c2.n_values == 4 and c2.categories is None
    c2.close()
    c9 = arr.facet_column(codes, n_values=9)
    got = arr.facets(strings, c9)
    assert got.counts.shape == (6, 9) and not got.counts[:, 4:].any() and np.array_equal(got.counts[:, :4], want()[2])
    c9.close()
    # errors
    with pytest.raises(ValueError, match="one entry per row"):
        arr.facet_column(codes[:-1])
    with pytest.raises(ValueError):
        arr.facet_column(codes, n_values=3)                      # a code >= n_values
    with pytest.raises(ValueError):
        arr.facet_column(np.where(codes < 0, -2, codes))         # a code < -1
    with pytest.raises(ValueError):
        arr.facet_column(codes.astype(np.float64))
    with pytest.raises(ValueError, match="slice"):
        arr[:100].facet_column(codes[:100])
    with pytest.raises(ValueError, match="slice"):
        arr[:100].facets(strings, col)
    with pytest.raises(ValueError, match="slice"):
        arr[:100].count(strings)
    with pytest.raises(TypeError):
        arr.facets(strings, col, devices=[0])
    with pytest.raises(TypeError):
        arr.count(strings, devices=[0])
    with pytest.raises(ValueError):
        arr.count(strings, mm=[1, 2])
    other = SearchArray.index(docs[:50])
    with pytest.raises(ValueError, match="another index"):
        other.facets(strings, col)
    col.close()
    with pytest.raises(ValueError, match="closed"):
        arr.facets(strings, col)


def test_error_paths(api, corpus):
    words, off, lens, orc = corpus
    codes, V = the_columns()["a"]
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    col = dev.facet_column(codes, V)
    i32p = _lib.ctypes.POINTER(_lib.ctypes.c_int32)

    def create(c, n_docs, n_values):
        h = _lib.ctypes.c_void_p()
        c = np.ascontiguousarray(c, dtype=np.int32)
        api.call("sa_codes_create", dev._h, c.ctypes.data_as(i32p), n_docs, n_values, _lib.ctypes.byref(h))
        api.sa_codes_destroy(h)

    # the C call checks the codes itself: a code >= n_values, a code < -1, another length, n_values out of range
    create(codes, N_DOCS, V)
    bad = codes.copy()
    bad[N_DOCS - 1] = V
    with pytest.raises(SearchArrayHipError, match=BAD_ARG):
        create(bad, N_DOCS, V)
    bad[N_DOCS - 1] = -2
    with pytest.raises(SearchArrayHipError, match=BAD_ARG):
        create(bad, N_DOCS, V)
    with pytest.raises(SearchArrayHipError, match=BAD_ARG):
        create(codes, N_DOCS - 1, V)
    for nv in (0, (1 << 20) + 1):
        with pytest.raises(SearchArrayHipError, match=BAD_ARG):
            create(np.full(N_DOCS, -1), N_DOCS, nv)
    # ... and so does the Python layer, before a launch
    for c, nv in ((bad, V), (codes[:-1], V), (codes, 0), (codes, (1 << 20) + 1), (codes.astype(np.float32), V), (codes.reshape(2, -1), V)):
        with pytest.raises(ValueError):
            dev.facet_column(c, nv)
    # phrase batches; tile sizes without a counting kernel
    pb = dev.phrase_batch([[0, 1], [2, 0]], k=5)
    with pytest.raises(SearchArrayHipError, match=UNSUPPORTED + ".*phrase"):
        pb.facet_counts(col)
    with pytest.raises(SearchArrayHipError, match=UNSUPPORTED + ".*phrase"):
        pb.facet_counts()
    pb.close()
    queries = head_queries(4)
    big = DeviceIndex(words, off, lens, tile_docs=16384, api=api)
    bt = big.batch(queries, k=10)
    bcol = big.facet_column(codes, V)
    with pytest.raises(SearchArrayHipError, match=UNSUPPORTED + ".*tile_docs"):
        bt.facet_counts(bcol)
    bt.run()                                                     # (the batch itself is as it was)
    assert (bt.fetch()[0] > 0).any()
    for x in (bcol, bt, big):
        x.close()
    # a column of another length; B x V above 2^28; not a column
    t5 = synth.corpus_triples(5, 10, 3, seed=1)
    w5, wt5 = rz.encode_sorted(t5[0], t5[1], t5[2])
    d5 = DeviceIndex(w5, rz.term_offsets(wt5, 10), t5[3], api=api)
    c5 = d5.facet_column([0, 1, -1, 1, 2], 3)
    bt = dev.batch(queries, k=10)
    with pytest.raises(SearchArrayHipError, match=BAD_ARG + ".*number of documents"):
        bt.facet_counts(c5)
    c5.close()
    d5.close()
    wide = dev.facet_column(np.full(N_DOCS, -1), 1 << 20)
    bt_big = dev.batch(np.zeros((257, 1), dtype=np.int64), k=1)
    with pytest.raises(SearchArrayHipError, match=BAD_ARG + ".*2\\^28"):
        bt_big.facet_counts(wide)
    bt_big.close()
    wide.close()
    with pytest.raises(TypeError):
        bt.facet_counts(codes)
    found, missing, counts = bt.facet_counts(col)                # after the rejected calls
    check((found, missing, counts), want_all(orc, queries, [[0] * 4] * 40, [0] * 40, codes, V), "after the rejected calls")
    col.close()
    with pytest.raises(ValueError, match="closed"):
        bt.facet_counts(col)
    bt.close()
    dev.close()


def test_the_new_calls_are_declared_and_bound():
    names = declared_functions()
    from tests.emu import emu_api
    for name in ("sa_codes_create", "sa_codes_destroy", "sa_batch_facet_counts", "sa_vec_facet_counts"):
        assert name in names and name in _lib.PROTOTYPES and hasattr(emu_api(), name)
    assert not any(n.startswith("sa_sharded") and "facet" in n for n in names), "the sharded handle has no such call"
