"""Filtered top-k: a BM25 batch that ranks inside a document filter (C ABI Part 2b, csrc/sa_filter.hip; Solr's `fq`).

Semantics under test: a filtered batch returns, per query, exactly the top-k of the UNFILTERED dense score with the scores of the
non-eligible documents set to 0 -- idf, average doc length and corpus size stay those of the whole index --, i.e.

    d = orc.score_terms_sum(q); d[~mask] = 0; O.topk(d, k)

bit for bit (scores and doc ids of the used slots, unused slots score 0 / doc 2**64-1), on every route the rule can pick for a
filtered batch, with the filter changed, cleared and closed under a live batch.  No tolerance anywhere: a filter must not change a
single score bit.  The tests assert themselves that they cannot pass by ignoring the filter (every query has a hit under every
non-empty filter; the filtered top-k differs from the unfiltered one for at least 30 of 40 queries)."""
import ctypes

import numpy as np
import pytest

from oracle import refimpl as O
from searcharray_amd import roaringish as rz, synth
from searcharray_amd._lib import SearchArrayHipError
from searcharray_amd.device_index import DeviceIndex, DocFilter
from searcharray_amd.postings import SearchArray
from searcharray_amd.sharded import ShardedIndex
from tests.helpers import set_opt
from tests.test_sharded import n_devices
from tests.test_stage import band_queries

N_DOCS, VOCAB = 9000, 400
NO_DOC = np.uint64(2**64 - 1)
HEADS = [0, 1, 2, 7, 350]
# the options that force each route; a filtered batch never runs dynamic pruning (it does not look at the filter): forced, it falls
# to the exhaustive kernels (grouped overlay + per-query tile kernel) and last_route() says "exhaustive"
ROUTES = {"stage": {"stage": 1}, "group": {"stage": 0, "sparse": 0, "group": 1}, "tiles": {"sparse": 0, "group": 0}, "sparse": {"sparse": 1}}


@pytest.fixture(scope="module")
def corpus():
    t, d, p, lens = synth.corpus_triples(N_DOCS, VOCAB, 14, seed=31)
    words, wt = rz.encode_sorted(t, d, p)
    return words, rz.term_offsets(wt, VOCAB), lens, O.OracleIndex.from_triples(t, d, p, N_DOCS, doc_lens=lens)


def the_masks():
    """random 50 %, 5 %, 0.5 % of the docs, the range [2048, 2348) (whole tiles empty on either side), nothing, everything"""
    rng = np.random.default_rng(5)
    out = {}
    for name, pct in (("50%", 50.0), ("5%", 5.0), ("0.5%", 0.5)):
        m = np.zeros(N_DOCS, dtype=bool)
        m[rng.choice(N_DOCS, size=int(N_DOCS * pct / 100), replace=False)] = True
        out[name] = m
    m = np.zeros(N_DOCS, dtype=bool)
    m[2048:2348] = True
    out["range"] = m
    out["empty"] = np.zeros(N_DOCS, dtype=bool)
    out["full"] = np.ones(N_DOCS, dtype=bool)
    return out


def queries_of(T, k, n=40):
    return band_queries(np.random.default_rng(100 + T + k), n, T, heads=HEADS)


def dense_scores(orc, queries):
    return [orc.score_terms_sum([int(x) for x in q if 0 <= int(x) < VOCAB]) for q in queries]


def want_topk(dense, mask, k):
    d = dense.copy()
    if mask is not None:
        d[~mask] = 0
    return O.topk(d, k)


def check_result(got, dense, mask, k, what, doc_base=0):
    """every query of the batch equals the oracle, bit for bit; returns how many queries have a hit / differ from the unfiltered top-k"""
    scores, docs = got
    hits = differ = 0
    for qi, d in enumerate(dense):
        ws, wd = want_topk(d, mask, k)
        n = int((ws > 0).sum())
        assert np.array_equal(scores[qi, :n], ws[:n]), f"{what}: q{qi} scores"
        assert np.array_equal(docs[qi, :n], wd[:n] + np.uint64(doc_base)), f"{what}: q{qi} docs"
        assert not scores[qi, n:].any() and (docs[qi, n:] == NO_DOC).all(), f"{what}: q{qi} unused slots"
        us, ud = want_topk(d, None, k)
        hits += n > 0
        differ += not (np.array_equal(us, ws) and np.array_equal(ud[us > 0], wd[ws > 0]))
    return hits, differ


def check_not_vacuous(name, hits, differ, n_queries, what):
    if name == "empty":
        assert hits == 0, f"{what}: the empty filter returned hits"
    elif name == "full":
        assert differ == 0, f"{what}: the full filter differs from the unfiltered result"
    else:
        assert hits == n_queries, f"{what}: only {hits} of {n_queries} queries have an eligible hit"
        assert differ >= 30, f"{what}: only {differ} of {n_queries} filtered top-k differ from the unfiltered ones"


# ---- 1. every route, forced
def route_cells(on_emu, route, tile):
    """(T, k) cells: all nine on the GPU; the host-emulated kernels take a diagonal (both tile-kernel selections and the staged route
    at every k and T once), thinner still for the second tile size and for forced pruning, which falls to the exhaustive kernels"""
    if not on_emu:
        return [(T, k) for T in (1, 4, 8) for k in (3, 50, 1000)]
    if tile != 1024:
        return [(4, 50)] if route != "sparse" else []
    return [(4, 3), (1, 50), (8, 1000)] if route != "sparse" else [(4, 3), (1, 50)]


@pytest.mark.parametrize("tile", [1024, 2048])
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_honours_the_filter(api, corpus, on_emu, route, tile):
    words, off, lens, orc = corpus
    masks = the_masks()
    dev = DeviceIndex(words, off, lens, tile_docs=tile, api=api)
    for T, k in route_cells(on_emu, route, tile):
        queries = queries_of(T, k)
        dense = dense_scores(orc, queries)
        must_stage = False
        if route == "stage":
            # every term staged is the staging load of a plan with zero starting bounds: where that is staged, the filtered run must be
            ref = dev.batch(queries, k=k, opts={"stage": 1, "stage_probe": 0})
            ref.run()
            must_stage = ref.last_route() == "staged"
            ref.close()
        bt = dev.batch(queries, k=k, opts=ROUTES[route])         # one batch per cell, the six filters through set_filter
        for name, mask in masks.items():
            what = f"{route} tile {tile} T {T} k {k} filter {name}"
            f = dev.doc_filter(mask=mask)
            assert f.count() == int(mask.sum())
            bt.set_filter(f)
            f.close()                                            # (the batch keeps it alive)
            for _ in range(2):                                   # the second run on the state the first one left
                bt.run()
            got_route = bt.last_route()
            assert got_route != "pruned", f"{what}: dynamic pruning does not look at the filter"
            if route == "stage":
                assert got_route == "staged" or not must_stage, f"{what}: route {got_route}"
            assert not bt.seeds().any(), f"{what}: a filtered run must not start from the corpus-wide bounds"
            hits, differ = check_result(bt.fetch(), dense, mask, k, what)
            check_not_vacuous(name, hits, differ, len(queries), what)
        bt.close()
    dev.close()


@pytest.mark.parametrize("route", ["stage", "tiles"])
def test_doc_base_and_global_row_ids(api, corpus, route):
    """a shard with doc_base = 50 000: from_rows takes GLOBAL ids (unsorted, with duplicates; ids of other shards are ignored) and
    the results carry global ids"""
    words, off, lens, orc = corpus
    base = 50_000
    dev = DeviceIndex(words, off, lens, tile_docs=1024, doc_base=base, api=api)
    mask = the_masks()["5%"]
    rng = np.random.default_rng(8)
    rows = np.flatnonzero(mask) + base
    rows = rng.permutation(np.concatenate([rows, rows[:50], [3, base - 1, base + N_DOCS, base + N_DOCS + 77, 2**40]]))
    f = dev.doc_filter(rows=rows)
    assert f.count() == int(mask.sum()) and np.array_equal(f.to_mask(), mask)
    queries = queries_of(4, 10)
    bt = dev.batch(queries, k=10, opts=ROUTES[route], filter=f)
    bt.run()
    hits, differ = check_result(bt.fetch(), dense_scores(orc, queries), mask, 10, f"doc_base {route}", doc_base=base)
    check_not_vacuous("5%", hits, differ, len(queries), f"doc_base {route}")
    bt.close()
    dev.close()


@pytest.mark.parametrize("tile", [4096, 8192])
def test_larger_tiles_fall_to_the_per_query_kernel(api, corpus, tile):
    """4096-doc tiles have a grouped kernel but no filtered instantiation of it, 8192-doc tiles have neither: group = 1 forced, a
    filtered batch runs the per-query tile kernel (whose summary test spans several 1024-doc blocks, past the shard's last one)"""
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=tile, api=api)
    queries = queries_of(4, 10)
    dense = dense_scores(orc, queries)
    bt = dev.batch(queries, k=10, opts=ROUTES["group"])
    for name in ("5%", "range", "empty"):
        mask = the_masks()[name]
        bt.set_filter(dev.doc_filter(mask=mask))
        bt.run()
        hits, differ = check_result(bt.fetch(), dense, mask, 10, f"tile {tile}, filter {name}")
        check_not_vacuous(name, hits, differ, len(queries), f"tile {tile}, filter {name}")
    bt.close()
    dev.close()


# ---- 2. the winners excluded: the case in which corpus-wide starting bounds are too high
@pytest.mark.parametrize("route", list(ROUTES))
def test_the_unfiltered_winners_excluded(api, corpus, route):
    words, off, lens, orc = corpus
    queries = queries_of(4, 10)
    dense = dense_scores(orc, queries)
    mask = np.ones(N_DOCS, dtype=bool)
    for d in dense:
        ws, wd = O.topk(d, 50)
        mask[wd[ws > 0].astype(np.int64)] = False
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    plain = dev.batch(queries, k=10, opts=ROUTES[route])
    had_seeds = plain.seeds().any()
    plain.close()
    assert had_seeds or route == "sparse", "the unfiltered batch of this set has starting bounds: the case is the sharp one"
    bt = dev.batch(queries, k=10, opts=ROUTES[route], filter=dev.doc_filter(mask=mask))
    assert not bt.seeds().any()
    for _ in range(2):
        bt.run()
    hits, differ = check_result(bt.fetch(), dense, mask, 10, f"winners excluded, {route}")
    assert hits == len(queries) and differ == len(queries)
    bt.close()
    dev.close()


# ---- 3. the life cycle of filters on one batch
@pytest.mark.parametrize("variant", ["plain", "cand_cap", "seed150"])
def test_filter_life_cycle_on_one_batch(api, corpus, variant):
    """unfiltered -> set_filter(f) -> run -> reset -> run -> step (idf table) -> set_filter(g) -> run -> set_filter(None) -> run, each
    result against its oracle.  cand_cap: candidate lists of 64 keys (the overflow / redo path, which must apply the filter);
    seed150: starting bounds 1.5 x too high on the unfiltered legs (flagged and redone; the filtered legs have no starting bounds)."""
    words, off, lens, orc = corpus
    if variant == "cand_cap":
        set_opt("SA_CAND_CAP", "64")
    if variant == "seed150":
        set_opt(seed_scale_pct=150)
    k = 50 if variant == "cand_cap" else 10
    masks = the_masks()
    qa, qb, qc = queries_of(4, k), band_queries(np.random.default_rng(1), 40, 4, HEADS), band_queries(np.random.default_rng(2), 40, 4, HEADS)
    da, db, dc = (dense_scores(orc, q) for q in (qa, qb, qc))
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    dev.set_idf_table(dev.idfs(np.arange(VOCAB)))
    never = dev.batch(qa, k=k)                                   # a batch that never sees a filter
    never.run()
    first = never.fetch()
    never.close()
    bt = dev.batch(qa, k=k)
    bt.run()
    got = bt.fetch()
    check_result(got, da, None, k, "unfiltered")
    assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])
    f = dev.doc_filter(mask=masks["50%"])
    g = dev.doc_filter(rows=np.flatnonzero(masks["5%"]))
    # a run nobody has fetched keeps the filter it ran with (none), whatever is set before the fetch
    bt.run(sync=False)
    bt.set_filter(f)
    check_result(bt.fetch(), da, None, k, "unfetched run, then set_filter")
    f.close()                                                    # closed before the batch's next run
    bt.run()
    check_result(bt.fetch(), da, masks["50%"], k, "set_filter(f)")
    bt.reset(qb)                                                 # the filter persists across reset and step
    bt.run(sync=False)
    check_result(bt.fetch(), db, masks["50%"], k, "reset under f")
    bt.step(np.ascontiguousarray(qc, dtype=np.uint32))
    check_result(bt.fetch(), dc, masks["50%"], k, "step under f")
    bt.set_filter(g)
    bt.run()
    hits, differ = check_result(bt.fetch(), dc, masks["5%"], k, "set_filter(g)")
    check_not_vacuous("5%", hits, differ, 40, "set_filter(g)")
    bt.set_filter(None)
    bt.run()
    check_result(bt.fetch(), dc, None, k, "set_filter(None)")
    bt.reset(qa)
    bt.run()
    last = bt.fetch()
    assert np.array_equal(last[0], first[0]) and np.array_equal(last[1], first[1]), "after the filters: what a batch that never saw one returns"
    g.close()
    bt.close()
    dev.close()


# ---- 4. filter objects
def test_filter_objects(api, corpus):
    words, off, lens, orc = corpus
    assert N_DOCS % 64 and N_DOCS % 1024                         # tail bits, a partial last tile
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    rng = np.random.default_rng(12)
    ma, mb = rng.random(N_DOCS) < 0.3, rng.random(N_DOCS) < 0.6
    ma[-1] = True
    mb[-1] = False
    a = dev.doc_filter(mask=ma)
    rows = np.flatnonzero(mb)
    b = dev.doc_filter(rows=rng.permutation(np.concatenate([rows, rows[::3], [N_DOCS, N_DOCS + 5, 2**33]])))
    assert isinstance(a, DocFilter) and a.count() == int(ma.sum()) and b.count() == int(mb.sum())
    assert np.array_equal(a.to_mask(), ma) and np.array_equal(b.to_mask(), mb)
    for got, want in (((a & b), ma & mb), ((a | b), ma | mb), ((a - b), ma & ~mb), ((~a), ~ma), ((~(a | ~a)), np.zeros(N_DOCS, bool))):
        assert got.count() == int(want.sum()) and np.array_equal(got.to_mask(), want)
        got.close()
    full = ~dev.doc_filter(mask=np.zeros(N_DOCS, bool))
    assert full.count() == N_DOCS                                # (the bits behind n_docs stay 0)
    for term in (0, 7, 350, VOCAB - 1):
        tf = dev.term_filter(term)
        want = dev.termfreqs_dense(term) > 0
        assert tf.count() == int(want.sum()) and np.array_equal(tf.to_mask(), want)
    for unknown in (VOCAB, -1, 2**31):
        assert dev.term_filter(unknown).count() == 0
    assert dev.doc_filter(rows=[]).count() == 0
    # errors: a mask of the wrong length, a filter of another index, a phrase batch
    with pytest.raises(ValueError):
        dev.doc_filter(mask=np.ones(N_DOCS - 1, bool))
    with pytest.raises(ValueError):
        dev.doc_filter()
    h = ctypes.c_void_p()
    one = np.ones(N_DOCS + 3, dtype=np.uint8)
    assert api.sa_filter_create_from_mask(dev._h, one.ctypes.data_as(ctypes.c_void_p), N_DOCS + 3, ctypes.byref(h)) != 0
    other = DeviceIndex(words, off, lens, tile_docs=2048, api=api)
    fo = other.doc_filter(mask=ma)
    bt = dev.batch(queries_of(4, 10), k=10)
    with pytest.raises(SearchArrayHipError, match="another index"):
        bt.set_filter(fo)
    with pytest.raises(SearchArrayHipError, match="different indexes"):
        a & fo
    with pytest.raises(TypeError):
        bt.set_filter(ma)
    pb = dev.phrase_batch([[0, 1], [2, 0]], k=5)
    with pytest.raises(SearchArrayHipError, match="phrase"):
        pb.set_filter(a)
    a.close()
    with pytest.raises(ValueError, match="closed"):
        a.count()
    pb.close()
    bt.close()
    other.close()
    dev.close()


# ---- 5. sharded
def test_sharded_filter_equals_the_single_index(api, corpus):
    words, off, lens, orc = corpus
    G = n_devices(api, 2)
    sh = ShardedIndex(words, off, lens, devices=list(range(G)), tile_docs=1024, api=api)
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    queries = queries_of(4, 10)
    dense = dense_scores(orc, queries)
    one_shard = np.zeros(N_DOCS, dtype=bool)                     # every eligible doc in ONE shard (the last one)
    one_shard[sh.bounds[-2] + 100: sh.bounds[-2] + 1900] = True
    sb = sh.batch(queries, k=10)
    bt = dev.batch(queries, k=10)
    for name, mask, as_rows in (("one shard", one_shard, False), ("5%", the_masks()["5%"], True)):
        fs = sh.doc_filter(rows=np.flatnonzero(mask)[::-1]) if as_rows else sh.doc_filter(mask=mask)
        assert fs.count() == int(mask.sum())
        sb.set_filter(fs)
        fs.close()
        bt.set_filter(dev.doc_filter(mask=mask))
        for b in (sb, bt):
            b.run()
        s1, d1 = sb.fetch()
        s2, d2 = bt.fetch()
        assert np.array_equal(s1, s2) and np.array_equal(d1, d2), f"sharded vs single index, filter {name}"
        hits, differ = check_result((s1, d1), dense, mask, 10, f"sharded, filter {name}")
        assert hits == len(queries) and differ >= 30
    sb.set_filter(None)
    sb.run()
    check_result(sb.fetch(), dense, None, 10, "sharded, filter cleared")
    with pytest.raises(ValueError):
        sh.doc_filter(mask=np.ones(N_DOCS + 1, bool))
    with pytest.raises(ValueError):
        sh.doc_filter(rows=[N_DOCS])
    sb.close()
    bt.close()
    dev.close()
    sh.close()


# ---- 6. SearchArray.search(filter=...)
def test_search_with_a_filter(default_api):
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(30)]
    p = 1.0 / np.arange(1, 31)
    p /= p.sum()
    docs = [" ".join(rng.choice(vocab, size=max(1, rng.poisson(12)), p=p)) for _ in range(700)]
    arr = SearchArray.index(docs)
    queries = [["w0", "w7", "w20"], "w3 w29", ["w1"], ["nope", "w2"], ["w5", "w5"]]
    mask = np.random.default_rng(4).random(700) < 0.2
    has_w3 = arr.termfreqs("w3") > 0
    unfiltered = arr.search(queries, k=7)

    def check(got, m, what):
        scores, ids = got
        for i, q in enumerate(queries):
            toks = q.split() if isinstance(q, str) else q
            dense = np.sum([arr.score(t) for t in toks], axis=0)
            dense[~m] = 0
            order = np.lexsort((np.arange(len(dense)), -dense))[:7]
            n = int((dense[order] > 0).sum())
            assert np.array_equal(ids[i, :n], order[:n].astype(np.uint64)) and np.allclose(scores[i, :n], dense[order][:n], rtol=1e-6), f"{what} q{i}"
            assert not scores[i, n:].any() and (ids[i, n:] == NO_DOC).all(), f"{what} q{i} unused slots"

    check(arr.search(queries, k=7, filter=mask), mask, "mask")
    assert not np.array_equal(arr.search(queries, k=7, filter=mask)[1], unfiltered[1])
    check(arr.search(queries, k=7, filter=np.flatnonzero(mask)[::-1]), mask, "row ids")
    f = arr.doc_filter(mask)
    check(arr.search(queries, k=7, filter=f), mask, "DocFilter")
    check(arr.search(queries, k=7, filter=f), mask, "DocFilter, reused")
    tf = arr.term_filter("w3")
    assert np.array_equal(tf.to_mask(), has_w3)
    check(arr.search(queries, k=7, filter=tf), has_w3, "term_filter")
    check(arr.search(queries, k=7, filter=f & tf), mask & has_w3, "DocFilter & term_filter")
    assert arr.term_filter("nope").count() == 0
    assert not arr.search(queries, k=7, filter=arr.term_filter("nope"))[0].any()
    check(arr.search(queries, k=7, filter=mask, devices=[0]), mask, "mask, devices=[0]")
    check(arr.search(queries, k=7, filter=f, devices=[0]), mask, "DocFilter, devices=[0]")
    got = arr.search(queries, k=7)                              # no filter: as before
    assert np.array_equal(got[0], unfiltered[0]) and np.array_equal(got[1], unfiltered[1])
    with pytest.raises(ValueError, match="slice"):
        arr[:10].search(queries, filter=mask[:10])
    with pytest.raises(ValueError, match="slice"):
        arr[:10].search(queries)
    with pytest.raises(ValueError):
        arr.search(queries, filter=np.ones(699, bool))
    with pytest.raises(ValueError):
        arr.search(queries, filter=np.asarray([0, 700]))
    with pytest.raises(ValueError):
        arr.search(queries, filter=np.asarray([-1, 5]))
    with pytest.raises(ValueError):
        arr.doc_filter(np.ones(701, bool))


# ---- 7. scale: the co-walking groups and the empty-tile skip over thousands of tiles
@pytest.mark.gpu
@pytest.mark.parametrize("k", [10, 100])
def test_filtered_batch_at_1m_docs(k):
    """1 M docs (the corpus of tests/test_config_scale.py), 256 four-term queries, default options (the library's own route rule),
    a random 10 % filter and one contiguous 1 % range: all 256 queries equal the oracle"""
    from searcharray_amd import _lib
    D, V = 1_000_000, 100_000
    api = _lib.api()
    lens, terms = synth.zipf_batch_tokens(0, D, V, fast=True)
    words, counts = synth.encode_batch(lens, terms, V)
    words, term_off = synth.concat_term_major([(words, counts)], V)
    doc_lens = lens.astype(np.float32)
    dev = DeviceIndex(words, term_off, doc_lens, api=api)
    orc = O.OracleIndex(words, np.arange(V), term_off, doc_lens, D)
    queries = synth.bm25_queries(256, vocab=V)
    dense = [orc.score_terms_sum([int(t) for t in q]) for q in queries]
    m10 = np.random.default_rng(5).random(D) < 0.10
    m1 = np.zeros(D, dtype=bool)
    m1[D // 3: D // 3 + D // 100] = True
    bt = dev.batch(queries, k=k)
    for name, mask in (("random 10 %", m10), ("contiguous 1 %", m1)):
        bt.set_filter(dev.doc_filter(mask=mask))
        for _ in range(2):
            bt.run()
        route = bt.last_route()
        scores, docs = bt.fetch()
        for qi, d in enumerate(dense):
            ws, wd = want_topk(d, mask, k)
            n = int((ws > 0).sum())
            assert np.array_equal(scores[qi, :n], ws[:n]) and np.array_equal(docs[qi, :n], wd[:n]), f"k {k}, filter {name}, route {route}: q{qi}"
            assert not scores[qi, n:].any(), f"k {k}, filter {name}, route {route}: q{qi} unused slots"
    bt.close()
    dev.close()
