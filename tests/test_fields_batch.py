"""device_index.FieldsBatch (Part 4b of the C ABI, csrc/sa_fields.hip): batches of multi-field term-centric queries at the C level.

Expected values never come from the code under test: every (field, term) score vector is `DeviceIndex.bm25_dense([term])` (times the
field's boost in float32), combined with numpy float64 in the order of `solr._term_centric` -- per clause the fields' vectors are
added left to right, maxed, `best + (total - best) * tie`; the clauses are added in order; rows that match fewer than `need` clauses
score 0 -- and ranked with the numpy selection of tests/test_solr_search.py (`yardstick`).  Every comparison is exact."""
import numpy as np
import pytest

from searcharray_amd import roaringish as rz
from searcharray_amd import synth
from searcharray_amd.device_index import NO_DOC, DeviceIndex, FieldsBatch
from tests.helpers import set_opt
from tests.test_solr_search import yardstick

N_DOCS, VOCAB = 4100, 50
K1 = [1.2, 0.9, 1.6]
B_ = [0.75, 0.4, 0.3]
BOOSTS = [3.0, None, 0.5]


def build(api, tiles, opts=None):
    devs = []
    for f, tile in enumerate(tiles):
        t, d, p, lens = synth.corpus_triples(N_DOCS, VOCAB - 5 * f, 3 + 5 * f, seed=20 + f)
        words, wt = rz.encode_sorted(t, d, p)
        devs.append(DeviceIndex(words, rz.term_offsets(wt, VOCAB - 5 * f), lens, tile_docs=tile, api=api, opts=opts))
    return devs


@pytest.fixture(scope="module")
def fields(api):
    """three indexes of 4100 docs per tile layout, and the dense score vector of every (field, term), computed once"""
    made = {}

    def get(tiles, opts=None):
        key = (tuple(tiles), None if opts is None else tuple(sorted(opts.items())))
        if key not in made:
            made[key] = build(api, tiles, opts)
        return made[key]

    vecs = {}
    ref = get((2048, 2048, 2048))                # (the score vectors do not depend on the tile size)

    def vec(f, term):
        if (f, term) not in vecs:
            if 0 <= term < ref[f].n_terms:
                v = ref[f].bm25_dense([term], k1=K1[f], b=B_[f])
                v = v * np.float32(BOOSTS[f]) if BOOSTS[f] is not None else v.copy()
            else:
                v = np.zeros(N_DOCS, dtype=np.float32)
            assert v.dtype == np.float32
            vecs[(f, term)] = v
        return vecs[(f, term)]

    yield get, vec
    for devs in made.values():
        for dev in devs:
            dev.close()


def weights_of(devs, terms):
    w = np.zeros(terms.shape, dtype=np.float32)
    for f, dev in enumerate(devs):
        w[:, :, f] = dev.idfs(terms[:, :, f].reshape(-1)).reshape(terms.shape[:2])
    return w


def expected_scores(vec, terms, need, tie):
    """float64[B][n_docs], combined as solr._term_centric combines"""
    B, T, F = terms.shape
    out = np.zeros((B, N_DOCS), dtype=np.float64)
    for q in range(B):
        clauses = np.zeros((T, N_DOCS), dtype=np.float64)
        for posn in range(T):
            stack = np.zeros((F + 1, N_DOCS), dtype=np.float64)
            for f in range(F):
                stack[f] = vec(f, int(terms[q, posn, f]))
            total = np.zeros(N_DOCS)
            for f in range(F):
                total += stack[f]
            best = stack.max(axis=0)
            clauses[posn] = best + (total - best) * tie
        enough = (clauses > 0).sum(axis=0) >= need[q]
        scores = np.sum(list(clauses), axis=0)
        scores[~enough] = 0
        out[q] = scores
    return out


def query_set(rng, B, T, rare=False):
    """term ids [B][T][3]: the same token position in every field (ids differ per field as vocabularies do), padding clauses, unknown ids"""
    terms = np.full((B, T, 3), -1, dtype=np.int64)
    for q in range(B):
        n = 1 + (q % T)
        for posn in range(n):
            for f in range(3):
                lo, hi = (25, VOCAB - 5 * f) if rare else (0, VOCAB - 5 * f)
                terms[q, posn, f] = rng.integers(lo, hi)
        if q % 5 == 3:
            terms[q, 0, 1] = 1000                # unknown in one field only
        if q % 7 == 6:
            terms[q, n - 1, :] = -1              # a clause no field knows
    need = np.asarray([1 + (q % 3 == 2) for q in range(B)], dtype=np.uint32)
    return terms, need


def check(fb, vec, terms, need, tie, k, mask, what):
    scores, rows, found = fb.fetch()
    want = expected_scores(vec, terms, need, tie)
    assert scores.dtype == np.float64 and rows.dtype == np.uint64 and scores.shape == (len(terms), k)
    for q in range(len(terms)):
        ws, wr, wf = yardstick(want[q], np.ones(N_DOCS, bool) if mask is None else mask, k)
        assert int(found[q]) == wf, f"{what} q{q}: found {found[q]} != {wf}"
        assert np.array_equal(rows[q], wr), f"{what} q{q}: rows differ"
        assert np.array_equal(scores[q], ws), f"{what} q{q}: scores differ"
    return want


@pytest.mark.parametrize("tiles", [(1024, 1024, 1024), (2048, 2048, 2048), (4096, 4096, 4096), (2048, 1024, 4096)],
                         ids=["1024", "2048", "4096", "mixed"])
def test_tile_sizes(api, fields, tiles):
    get, vec = fields
    devs = get(tiles)
    assert [dev.info().tile_docs for dev in devs] == list(tiles) and all(dev.n_docs == N_DOCS for dev in devs)
    terms, need = query_set(np.random.default_rng(3), 7, 3)
    fb = FieldsBatch(devs, K1, B_, BOOSTS)
    try:
        for k, tie in ((10, 0.1), (1000, 1.0)):
            fb.set_queries(terms, weights_of(devs, terms), need, k=k, tie=tie)
            fb.run()
            want = check(fb, vec, terms, need, tie, k, None, f"tiles {tiles} k={k}")
            pos = (want > 0).sum(axis=1)
            assert pos.max() > 1000 and pos.min() < 1000 and (pos == 0).any()      # selection, padding and an empty result all occur
            assert any(len(np.unique(w[w > 0])) < (w > 0).sum() for w in want)     # ties
        mask = np.zeros(N_DOCS, dtype=bool)
        mask[2048:3000] = True                   # whole tiles of every size stay empty
        filt = devs[1].doc_filter(mask=mask)     # (a filter of ANY of the indexes)
        try:
            fb.set_filter(filt)
            fb.run()
            check(fb, vec, terms, need, 1.0, 1000, mask, f"tiles {tiles} filtered")
            fb.set_filter(None)
            fb.run()
            check(fb, vec, terms, need, 1.0, 1000, None, f"tiles {tiles} filter cleared")
        finally:
            filt.close()
    finally:
        fb.close()


def test_terms_with_and_without_directory_rows(api, fields):
    get, vec = fields
    devs = get((2048, 2048, 2048), {"dir_div": -200})       # rows for df >= 200 x 3 tiles only
    terms, need = query_set(np.random.default_rng(5), 6, 4)
    rowed = []
    for f, dev in enumerate(devs):
        info = dev.info()
        assert info.n_tiles == 3
        df = dev.docfreqs()
        assert info.n_dir_terms == int((df >= 600).sum())
        used = np.unique(terms[:, :, f][(terms[:, :, f] >= 0) & (terms[:, :, f] < dev.n_terms)])
        rowed += [bool(df[t] >= 600) for t in used]
    assert any(rowed) and not all(rowed)                    # both ways to a tile's slice are taken
    fb = FieldsBatch(devs, K1, B_, BOOSTS)
    try:
        fb.set_queries(terms, weights_of(devs, terms), need, k=100, tie=0.3)
        fb.run()
        check(fb, vec, terms, need, 0.3, 100, None, "dir_div")
    finally:
        fb.close()


def test_reuse_many_hits_then_few(api, fields):
    get, vec = fields
    devs = get((2048, 2048, 2048))
    rng = np.random.default_rng(9)
    many, need_many = query_set(rng, 9, 4)
    few, need_few = query_set(rng, 5, 2, rare=True)
    need_few[:] = 2                                         # (rare terms, both clauses: few rows or none)
    fb = FieldsBatch(devs, K1, B_, BOOSTS)
    try:
        fb.set_queries(many, weights_of(devs, many), need_many, k=100, tie=0.5)
        fb.run()
        first = check(fb, vec, many, need_many, 0.5, 100, None, "first set")
        fb.set_queries(few, weights_of(devs, few), need_few, k=50, tie=0.0)
        fb.run(sync=False)
        second = check(fb, vec, few, need_few, 0.0, 50, None, "second set")
        assert (first > 0).sum(axis=1).max() > 2000 and (second > 0).sum(axis=1).max() < 600    # (every slot of the second run is checked, past its hits too)
        assert ((second > 0).sum(axis=1) == 0).any()
        fb.set_queries(many, weights_of(devs, many), need_many, k=100, tie=0.5)                    # and back
        fb.run()
        check(fb, vec, many, need_many, 0.5, 100, None, "first set again")
    finally:
        fb.close()


def test_slices_of_queries_equal_one_launch(api, fields):
    get, vec = fields
    devs = get((2048, 2048, 2048))
    terms, need = query_set(np.random.default_rng(13), 65, 3)
    w = weights_of(devs, terms)
    whole = FieldsBatch(devs, K1, B_, BOOSTS)
    set_opt("fields_cand_mb", 1)                            # 3 tiles x 1000 candidates x 12 bytes per query: 29 queries per slice
    sliced = FieldsBatch(devs, K1, B_, BOOSTS)
    try:
        results = []
        for fb in (whole, sliced):
            fb.set_queries(terms, w, need, k=1000, tie=0.1)
            fb.run()
            results.append(fb.fetch())
        assert whole.profile()[2] == 1 and sliced.profile()[2] >= 3
        assert whole.profile()[1] == sliced.profile()[1] > 0
        for a, b in zip(*results):
            assert np.array_equal(a, b)
        check(sliced, vec, terms, need, 0.1, 1000, None, "sliced")
    finally:
        whole.close()
        sliced.close()


def test_argument_errors(api, fields):
    from searcharray_amd._lib import SearchArrayHipError
    get, vec = fields
    devs = get((2048, 2048, 2048))
    t, d, p, lens = synth.corpus_triples(100, 20, 4, seed=1)
    words, wt = rz.encode_sorted(t, d, p)
    short = DeviceIndex(words, rz.term_offsets(wt, 20), lens, api=api)
    try:
        with pytest.raises(SearchArrayHipError, match="different numbers of documents"):
            FieldsBatch([devs[0], short], [1.2, 1.2], [0.75, 0.75])
        with pytest.raises(SearchArrayHipError, match="1 .. 8"):
            FieldsBatch([short] * 9, [1.2] * 9, [0.75] * 9)
        fb = FieldsBatch(devs, K1, B_, BOOSTS)
        try:
            with pytest.raises(SearchArrayHipError, match="no query set"):
                fb.run()
            terms, need = query_set(np.random.default_rng(1), 2, 2)
            with pytest.raises(ValueError, match="k must be"):
                fb.set_queries(terms, weights_of(devs, terms), need, k=1025)
            filt = short.doc_filter(mask=np.ones(100, bool))
            try:
                with pytest.raises(SearchArrayHipError, match="another number of documents"):
                    fb.set_filter(filt)
            finally:
                filt.close()
        finally:
            fb.close()
        set_opt("impact", 0)                                # no impact stream: the caller answers query by query
        with pytest.raises(SearchArrayHipError, match="no impact stream"):
            FieldsBatch(devs, K1, B_, BOOSTS)
    finally:
        short.close()
    assert NO_DOC == 2**64 - 1
