"""Document filters for phrase batches (sa_phrase_batch_set_filter; `SearchArray.search_phrases(filter=...)`).

Semantics under test -- the contract of the BM25 batches' filters (tests/test_filter.py): for every phrase of a batch the result is exactly

    d = orc.score(phrase, slop=slop); d[~mask] = 0; O.topk(d, k)

bit for bit (scores and doc ids of the used slots, unused slots score 0 / doc 2**64-1), at every site at which a phrase batch ranks:
the tile kernel (exact phrases of distinct terms, whole and middle-out plans), inside the doc-parallel span kernel, the shared ranking
launch over the slop phrases' count vectors, and the one-by-one ranking of the dense route (repeated terms, more than 18 terms, slop
phrases the shared launches decline) -- with the filter changed, cleared and closed under a live batch.  No tolerance anywhere.  The
tests assert themselves that they cannot pass by ignoring the filter: at least 30 phrases of the set have 200 matches or more, each of
them has an eligible hit under every non-empty mask, and the filtered top-k differs from the unfiltered one for at least 25 of them."""
import ctypes
import re

import numpy as np
import pytest

from oracle import refimpl as O
from searcharray_amd import roaringish as rz, synth
from searcharray_amd._lib import SearchArrayHipError
from searcharray_amd.device_index import DeviceIndex
from searcharray_amd.postings import SearchArray
from searcharray_amd.sharded import ShardedIndex
from tests.helpers import golden_corpus
from tests.test_sharded import n_devices

N_DOCS, VOCAB = 9000, 60                                         # 5 phrase tiles of 2048 docs, or 3 of 4096 (a ragged last one)
NO_DOC = np.uint64(2**64 - 1)
KS = (3, 10, 100)                                                # (k <= 32 and k > 32 differ in the span kernel's compaction)
MIDDLE_OUT = [0, 1, 5, 2, 3]                                     # the shortest list strictly inside: counted as min(left, right)
# the options that force each slop route (csrc/sa_spans.hip, sa_span_counts_batch)
SLOP_ROUTES = {"default": {}, "span_doc_multi=0": {"span_doc_multi": 0}, "span_doc_rank=0": {"span_doc_rank": 0},
               "span_doc=0": {"span_doc": 0}, "span_multi=0": {"span_multi": 0}}


def the_phrases():
    """(terms, slop) x 40: the seeded recipe -- exact pairs and triples (the tile kernel), slop pairs and triples, a four-term slop
    phrase, repeated terms with and without slop -- and three more that may match little or nothing: the middle-out plan, 19 terms,
    an unknown term"""
    rng = np.random.default_rng(41)
    out = [([int(x) for x in rng.choice(10, 2, replace=False)], 0) for _ in range(14)]
    out += [([int(x) for x in rng.choice(6, 3, replace=False)], 0) for _ in range(6)]
    for _ in range(8):
        ph = [int(x) for x in rng.choice(20, 2, replace=False)]
        out.append((ph, int(rng.integers(1, 4))))
    for _ in range(4):
        ph = [int(x) for x in rng.choice(12, 3, replace=False)]
        out.append((ph, int(rng.integers(1, 4))))
    out += [([1, 2, 0, 3], 3), ([0, 0], 0), ([0, 0, 1], 0), ([1, 0, 1, 0], 0), ([0, 1, 0], 2)]
    assert len(out) == 37
    return out + [(MIDDLE_OUT, 0), (list(range(19)), 0), ([1, VOCAB + 39], 0)]


def the_masks(n=N_DOCS):
    """random 50 % and 5 % of the docs, the range [2048, 2348) (whole tiles empty on both sides at either tile size), nothing, everything"""
    rng = np.random.default_rng(5)
    out = {}
    for name, pct in (("50%", 50.0), ("5%", 5.0)):
        m = np.zeros(n, dtype=bool)
        m[rng.choice(n, size=int(n * pct / 100), replace=False)] = True
        out[name] = m
    m = np.zeros(n, dtype=bool)
    m[2048:2348] = True
    out["range"] = m
    out["empty"] = np.zeros(n, dtype=bool)
    out["full"] = np.ones(n, dtype=bool)
    return out


def dense_scores(orc, phrases, n_docs, vocab):
    return [orc.score(list(ph), slop=sl) if all(0 <= t < vocab for t in ph) else np.zeros(n_docs, np.float32) for ph, sl in phrases]


@pytest.fixture(scope="module")
def corpus():
    """the index arrays, the oracle, the phrase set, its dense oracle scores (computed once, never written to) and the live phrases"""
    t, d, p, lens = synth.corpus_triples(N_DOCS, VOCAB, 45, seed=3)
    words, wt = rz.encode_sorted(t, d, p)
    off = rz.term_offsets(wt, VOCAB)
    orc = O.OracleIndex.from_triples(t, d, p, N_DOCS, doc_lens=lens)
    phrases = the_phrases()
    dense = dense_scores(orc, phrases, N_DOCS, VOCAB)
    for x in dense:
        x.setflags(write=False)
    live = [i for i in range(37) if int((dense[i] > 0).sum()) >= 200]        # (the three added phrases are exempt)
    assert len(live) >= 30, f"only {len(live)} live phrases"
    lens_w = np.diff(off.astype(np.int64))
    assert 1 < int(np.argmin(lens_w[MIDDLE_OUT])) < len(MIDDLE_OUT) - 2, "the middle-out phrase takes the two-part plan"
    return words, off, lens, orc, phrases, dense, live


# the set without the three slop phrases over the most frequent terms (cells: why): what the tests beside the forced routes run
HEAVY = (30, 32, 36)


def light(corpus):
    words, off, lens, orc, phrases, dense, live = corpus
    keep = [i for i in range(len(phrases)) if i not in HEAVY]
    assert [phrases[i] for i in HEAVY] == [([2, 0, 3], 3), ([1, 2, 0, 3], 3), ([0, 1, 0], 2)]
    return [phrases[i] for i in keep], [dense[i] for i in keep], [keep.index(i) for i in live if i not in HEAVY]


def make_batch(dev, phrases, k, opts=None, **kw):
    return dev.phrase_batch([ph for ph, _ in phrases], k=k, slop=[sl for _, sl in phrases], opts=opts, **kw)


def want_topk(dense, mask, k):
    d = dense.copy()
    if mask is not None:
        d[~mask] = 0
    return O.topk(d, k)


def check_result(got, dense, mask, k, what, live=(), doc_base=0):
    """every phrase of the batch equals the oracle, bit for bit; returns how many LIVE phrases have a hit / differ from the unfiltered top-k"""
    scores, docs = got
    hits = differ = 0
    for i, d in enumerate(dense):
        ws, wd = want_topk(d, mask, k)
        n = int((ws > 0).sum())
        assert np.array_equal(scores[i, :n], ws[:n]), f"{what}: phrase {i} scores"
        assert np.array_equal(docs[i, :n], wd[:n] + np.uint64(doc_base)), f"{what}: phrase {i} docs"
        assert not scores[i, n:].any() and (docs[i, n:] == NO_DOC).all(), f"{what}: phrase {i} unused slots"
        if i in live:
            us, ud = want_topk(d, None, k)
            hits += n > 0
            differ += not (np.array_equal(us, ws) and np.array_equal(ud[us > 0], wd[ws > 0]))
    return hits, differ


def check_not_vacuous(name, got, hits, differ, n_live, what):
    if name == "empty":
        assert not got[0].any() and (got[1] == NO_DOC).all(), f"{what}: the empty filter returned hits"
    elif name == "full":
        assert differ == 0, f"{what}: the full filter differs from the unfiltered result"
    else:
        assert hits == n_live, f"{what}: only {hits} of {n_live} live phrases have an eligible hit"
        assert differ >= 25, f"{what}: only {differ} of {n_live} filtered top-k differ from the unfiltered ones"


def ranked_by(err):
    """the last run's phrases per ranking site, from the library's trace line"""
    m = re.findall(r"sa_phrase_batch: ranked (\d+) phrases by the tile kernel, (\d+) inside the span kernel, (\d+) by the shared ranking launch, "
                   r"(\d+) one by one( \(filtered\))?", err)
    assert m, err[-2000:]
    tile, fused, shared, single = (int(x) for x in m[-1][:4])
    return {"tile": tile, "fused": fused, "shared": shared, "single": single, "filtered": bool(m[-1][4])}


# ---- 1. every ranking site, forced
MASK_NAMES = ("50%", "5%", "range", "empty", "full")


def cells(on_emu, ptile, docdir, route):
    """(k, ((mask, runs), ...)) per batch: every k, all five masks and two runs per filter on the GPU, the whole set in one batch.
    Three phrases of the set -- the slop phrases over the most frequent terms, which take the five-stage shared launches -- cost the
    host-emulated span machines 70 s per RUN whatever the filter, so the emulator runs the set without them (light(): a run takes
    a few seconds) on a diagonal of the grid: both tile sizes, the compacted (k <= 32) and the uncompacted span kernel, a second
    run, whole tiles empty, the empty filter, and the routes that rank inside the span kernel, through count vectors and one by one"""
    if not on_emu:
        return [(k, tuple((m, 2) for m in MASK_NAMES)) for k in KS]
    if (ptile, docdir, route) == (2048, 1, "default"):
        return [(10, (("50%", 2), ("range", 1)))]
    if (ptile, docdir, route) == (4096, 1, "span_doc_rank=0"):
        return [(100, (("5%", 1), ("empty", 1)))]
    if (ptile, docdir, route) == (4096, 0, "default"):
        return [(100, (("range", 1),))]
    if (ptile, docdir, route) in ((2048, 1, "span_doc_multi=0"), (2048, 1, "span_doc=0")):
        return [(3, (("5%", 1),))]
    return []


@pytest.mark.parametrize("route", list(SLOP_ROUTES))
@pytest.mark.parametrize("docdir", [1, 0])
@pytest.mark.parametrize("ptile", [2048, 4096])
def test_every_ranking_site_honours_the_filter(api, corpus, on_emu, capfd, ptile, docdir, route):
    words, off, lens, orc, phrases, dense, live = corpus
    if on_emu:
        phrases, dense, live = light(corpus)
    masks = the_masks()
    if not cells(on_emu, ptile, docdir, route):
        return
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    n_dense = sum(1 for ph, sl in phrases if sl > 0 or len(set(ph)) < len(ph) or len(ph) > 18)
    for k, plan in cells(on_emu, ptile, docdir, route):
        bt = make_batch(dev, phrases, k, opts=dict(SLOP_ROUTES[route], ptile=ptile, phrase_docdir=docdir, trace=1))
        for name, runs in plan:                                  # one batch per cell, the filters through set_doc_filter
            mask = masks[name]
            what = f"ptile {ptile} docdir {docdir} {route} k {k} filter {name}"
            f = dev.doc_filter(mask=mask)
            bt.set_doc_filter(f)
            f.close()                                            # (the batch keeps it alive)
            for _ in range(runs):                                # the second run on the state the first one left
                capfd.readouterr()
                bt.run()
                got = bt.fetch()
                by = ranked_by(capfd.readouterr().err)
                hits, differ = check_result(got, dense, mask, k, what, live)
                check_not_vacuous(name, got, hits, differ, len(live), what)
            # the sites that ranked: the tile kernel the exact phrases of distinct terms, the rest by the route that was forced
            assert by["filtered"] and by["tile"] == len(phrases) - n_dense, (what, by)
            assert by["fused"] + by["shared"] + by["single"] == n_dense and by["single"] >= 4, (what, by)   # (repeated terms, 19 terms: one by one)
            if route == "default":
                assert by["fused"] >= 1, (what, by)              # the span kernel ranked slop phrases itself
                assert by["shared"] >= 1 or on_emu, (what, by)   # ... and the three over the most frequent terms went through count vectors
            elif route == "span_multi=0":
                assert by["fused"] == 0 and by["shared"] == 0, (what, by)
            else:
                assert by["fused"] == 0 and by["shared"] >= 1, (what, by)      # count vectors, ranked by the shared launch
        bt.close()
    dev.close()


# ---- 2. clean state after a filtered run
@pytest.mark.parametrize("route", ["default", "span_doc_rank=0", "span_doc_multi=0"])
def test_filtered_runs_leave_the_count_vectors_clean(api, corpus, on_emu, route):
    """the shared ranking launch puts the pooled count vectors back to zeros -- also for excluded docs and for tiles whose filter
    blocks are empty: the same batch unfiltered afterwards, and a fresh batch of OTHER slop phrases on the index, equal the oracle"""
    words, off, lens, orc = corpus[:4]
    phrases, dense, live = light(corpus)
    masks = the_masks()
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    k = 10
    bt = make_batch(dev, phrases, k, opts=SLOP_ROUTES[route])
    for name in ("range",) if on_emu else ("range", "5%", "empty"):      # (the emulator: the mask that leaves whole tiles empty)
        bt.set_doc_filter(dev.doc_filter(mask=masks[name]))
        bt.run()
        got = bt.fetch()
        hits, differ = check_result(got, dense, masks[name], k, f"{route}, filter {name}", live)
        check_not_vacuous(name, got, hits, differ, len(live), f"{route}, filter {name}")
        bt.set_doc_filter(None)
        for _ in range(1 if on_emu else 2):
            bt.run()
            check_result(bt.fetch(), dense, None, k, f"{route}, cleared after {name}")
        rng = np.random.default_rng(77)
        others = [([int(x) for x in 4 + rng.choice(16, T, replace=False)], int(rng.integers(1, 4))) for T in (2, 2, 3, 2, 4, 3)]
        fresh = make_batch(dev, others, k, opts=SLOP_ROUTES[route])
        fresh.run()
        check_result(fresh.fetch(), dense_scores(orc, others, N_DOCS, VOCAB), None, k, f"{route}, a fresh batch after {name}")
        fresh.close()
    bt.close()
    dev.close()


# ---- 3. reset keeps the filter; filters swapped between runs
def test_reset_keeps_the_filter(api, corpus):
    words, off, lens, orc = corpus[:4]
    phrases, dense, live = light(corpus)
    masks = the_masks()
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    k = 10
    n = len(phrases)
    set_a, set_b = phrases, phrases[18:] + phrases[:18]          # (the same number of phrases, none longer than the batch's)
    da, db = dense, dense[18:] + dense[:18]
    fa, fb = dev.doc_filter(mask=masks["50%"]), dev.doc_filter(rows=np.flatnonzero(masks["range"]))
    bt = make_batch(dev, set_a, k, filter=fa)
    fa.close()
    bt.run()
    check_result(bt.fetch(), da, masks["50%"], k, "filter A")
    bt.reset([ph for ph, _ in set_b], slop=[sl for _, sl in set_b])
    bt.run()
    live_b = [(i - 18) % n for i in live]
    hits, differ = check_result(bt.fetch(), db, masks["50%"], k, "reset under filter A", live_b)
    assert hits == len(live) and differ >= 25, (hits, differ)
    bt.run(sync=False)                                           # a run in flight while the filter is replaced
    bt.set_doc_filter(fb)
    check_result(bt.fetch(), db, masks["50%"], k, "a run enqueued before the filter was replaced")
    bt.run()
    hits, differ = check_result(bt.fetch(), db, masks["range"], k, "filter B", live_b)
    assert hits == len(live) and differ >= 25, (hits, differ)
    fb.close()
    bt.set_doc_filter(None)
    bt.set_doc_filter(None)
    bt.run()
    check_result(bt.fetch(), db, None, k, "no filter")
    bt.close()
    dev.close()


# ---- 4. doc_base
def test_doc_base_and_global_ids(api):
    """an index with doc_base = 50 000: the filter's bits are shard-local (from_rows takes GLOBAL ids), the results carry global ids"""
    g, (t, d, p), lens, num_docs, vocab = golden_corpus("zipf_small")
    words, wt = rz.encode_sorted(t, d, p)
    orc = O.OracleIndex.from_triples(t, d, p, num_docs, doc_lens=lens)
    base = 50_000
    dev = DeviceIndex(words, rz.term_offsets(wt, vocab), lens, tile_docs=1024, api=api, doc_base=base)
    phrases = [([0, 1], 0), ([1, 0], 0), ([2, 0, 1], 0), ([0, 1], 2), ([3, 1, 2], 2), ([0, 0], 0), ([1, 2], 0), ([2, 1], 1)]
    dense = dense_scores(orc, phrases, num_docs, vocab)
    mask = np.random.default_rng(5).random(num_docs) < 0.3
    rows = np.concatenate([np.flatnonzero(mask)[::-1] + base, [3, base - 1, base + num_docs, 2**40]])
    f = dev.doc_filter(rows=rows)
    assert np.array_equal(f.to_mask(), mask)
    k = 10
    bt = make_batch(dev, phrases, k, filter=f)
    for _ in range(2):
        bt.run()
    every = list(range(len(phrases)))
    hits, differ = check_result(bt.fetch(), dense, mask, k, "doc_base", every, doc_base=base)
    assert hits >= 6 and differ >= 6, (hits, differ)
    bt.close()
    dev.close()


# ---- 5. errors
def test_errors(api, corpus):
    words, off, lens, orc, phrases, dense, live = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    other = DeviceIndex(words, off, lens, tile_docs=2048, api=api)
    f, fo = dev.doc_filter(mask=the_masks()["5%"]), other.doc_filter(mask=the_masks()["5%"])
    pb = dev.phrase_batch([[0, 1], [2, 0]], k=5)
    with pytest.raises(SearchArrayHipError, match="another index"):
        pb.set_doc_filter(fo)
    with pytest.raises(SearchArrayHipError, match="another index"):
        dev.phrase_batch([[0, 1]], k=5, filter=fo)
    with pytest.raises(TypeError):
        pb.set_doc_filter(the_masks()["5%"])
    with pytest.raises(SearchArrayHipError, match="phrase"):     # (the BM25 batches' call keeps refusing a phrase handle)
        pb.set_filter(f)
    bm = dev.batch(np.asarray([[0, 1], [2, 3]]), k=5)
    assert api.sa_phrase_batch_set_filter(bm._h, f._need()) != 0
    with pytest.raises(SearchArrayHipError, match="phrase batch"):
        api.call("sa_phrase_batch_set_filter", bm._h, f._need())
    assert api.sa_phrase_batch_set_filter(None, f._need()) != 0
    f.close()
    with pytest.raises(ValueError, match="closed"):
        pb.set_doc_filter(f)
    # k and the other arguments are checked as before
    with pytest.raises(Exception, match="k must be"):
        dev.phrase_batch([[0, 1]], k=0, filter=None)
    with pytest.raises(Exception, match="at least two terms"):
        dev.phrase_batch([[0]], k=3)
    with pytest.raises(ValueError, match="slop"):
        dev.phrase_batch([[0, 1]], k=3, slop=-1)
    for h in (bm, pb):
        h.close()
    other.close()
    dev.close()


# ---- 6. sharded
def test_sharded_phrase_filter_equals_the_single_index(api, corpus, on_emu):
    words, off, lens, orc = corpus[:4]
    phrases, dense, live = light(corpus)
    G = n_devices(api, 2)
    sh = ShardedIndex(words, off, lens, devices=list(range(G)), tile_docs=1024, api=api)
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    masks = the_masks()
    one_shard = np.zeros(N_DOCS, dtype=bool)                     # every eligible doc in ONE shard (the last one)
    one_shard[sh.bounds[-2] + 100: sh.bounds[-2] + 1900] = True
    k = 10
    ph, sl = [p_ for p_, _ in phrases], [s_ for _, s_ in phrases]
    f0 = sh.doc_filter(mask=masks["50%"])
    sb = sh.phrase_batch(ph, k=k, slop=sl, filter=f0)
    f0.close()
    bt = make_batch(dev, phrases, k, filter=dev.doc_filter(mask=masks["50%"]))
    legs = [("50%", masks["50%"], None), ("one shard", one_shard, False), ("5%", masks["5%"], True)]
    for name, mask, as_rows in legs[:2] if on_emu else legs:
        if as_rows is not None:
            fs = sh.doc_filter(rows=np.flatnonzero(mask)[::-1]) if as_rows else sh.doc_filter(mask=mask)
            assert fs.count() == int(mask.sum())
            sb.set_doc_filter(fs)
            fs.close()
            bt.set_doc_filter(dev.doc_filter(mask=mask))
        for b in (sb, bt):
            b.run()
        s1, d1 = sb.fetch()
        s2, d2 = bt.fetch()
        assert np.array_equal(s1, s2) and np.array_equal(d1, d2), f"sharded vs single index, filter {name}"
        hits, differ = check_result((s1, d1), dense, mask, k, f"sharded, filter {name}", live)
        assert hits == len(live) and differ >= 25, (name, hits, differ)
    sb.set_doc_filter(None)
    sb.run()
    check_result(sb.fetch(), dense, None, k, "sharded, filter cleared")
    with pytest.raises(TypeError):
        sb.set_doc_filter(dev.doc_filter(mask=masks["5%"]))
    qb = sh.batch(np.asarray([[0, 1]]), k=3)
    with pytest.raises(ValueError):
        qb.set_doc_filter(None)
    qb.close()
    sb.close()
    bt.close()
    dev.close()
    sh.close()


# ---- 7. SearchArray.search_phrases(filter=...)
def test_search_phrases_with_a_filter(default_api):
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(12)]
    p = 1.0 / np.arange(1, 13)
    p /= p.sum()
    docs = [" ".join(rng.choice(vocab, size=max(2, rng.poisson(14)), p=p)) for _ in range(700)]
    arr = SearchArray.index(docs)
    phrases = [["w0", "w1"], ["w1", "w0", "w2"], ["w0", "w0"], ["w2", "w0"], ["nope", "w1"], ["w3", "w1"], ["w0", "w1", "w0"]]
    slops = [0, 0, 0, 2, 0, 3, 1]
    k = 7
    mask = np.random.default_rng(4).random(700) < 0.2
    has_w3 = arr.termfreqs("w3") > 0
    unfiltered = arr.search_phrases(phrases, k=k, slop=slops)

    def check(got, m, what):
        scores, ids = got
        for i, (ph, sl) in enumerate(zip(phrases, slops)):
            dense = np.asarray(arr.score(ph, slop=sl), dtype=np.float32).copy()
            dense[~m] = 0
            ws, wd = O.topk(dense, k)
            n = int((ws > 0).sum())
            assert np.array_equal(scores[i, :n], ws[:n]) and np.array_equal(ids[i, :n], wd[:n]), f"{what}: phrase {i}"
            assert not scores[i, n:].any() and (ids[i, n:] == NO_DOC).all(), f"{what}: phrase {i} unused slots"

    check(unfiltered, np.ones(700, bool), "no filter")
    got = arr.search_phrases(phrases, k=k, slop=slops, filter=mask)
    check(got, mask, "mask")
    assert not np.array_equal(got[1], unfiltered[1])
    check(arr.search_phrases(phrases, k=k, slop=slops, filter=np.flatnonzero(mask)[::-1]), mask, "row ids")
    f = arr.doc_filter(mask)
    check(arr.search_phrases(phrases, k=k, slop=slops, filter=f), mask, "DocFilter")
    check(arr.search_phrases(phrases, k=k, slop=slops, filter=f), mask, "DocFilter, reused")
    tf = arr.term_filter("w3")
    check(arr.search_phrases(phrases, k=k, slop=slops, filter=tf), has_w3, "term_filter")
    check(arr.search_phrases(phrases, k=k, slop=slops, filter=f & tf), mask & has_w3, "DocFilter & term_filter")
    assert not arr.search_phrases(phrases, k=k, slop=slops, filter=arr.term_filter("nope"))[0].any()
    for what, flt in (("mask", mask), ("DocFilter", f)):
        one = arr.search_phrases(phrases, k=k, slop=slops, filter=flt)
        sharded = arr.search_phrases(phrases, k=k, slop=slops, filter=flt, devices=[0])
        check(sharded, mask, f"{what}, devices=[0]")
        assert np.array_equal(one[0], sharded[0]) and np.array_equal(one[1], sharded[1]), what
    again = arr.search_phrases(phrases, k=k, slop=slops)        # no filter: as before
    assert np.array_equal(again[0], unfiltered[0]) and np.array_equal(again[1], unfiltered[1])
    with pytest.raises(ValueError, match="slice"):
        arr[:10].search_phrases(phrases, filter=mask[:10])
    with pytest.raises(ValueError):
        arr.search_phrases(phrases, filter=np.ones(699, bool))
    with pytest.raises(ValueError):
        arr.search_phrases(phrases, filter=np.asarray([0, 700]))
