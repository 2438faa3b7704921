"""The staged-tile kernel's candidate list and who owns a candidate (csrc/sa_stage.hip): the query threads lay the postings of
every query's essential positions out as one list per tile -- the concatenation of SEGMENTS, the slice of one essential position of one
query -- and a lane of stage A finds, for candidate number x, its query, position and posting (`owner_of`: a search of the queries' first
candidates, then of the query's positions).  Stage A takes the list in rounds of 1024 candidates, a wave 64 of them; stage B's rounds
fill the list of finalists.

The cases are the smallest shapes at which that resolution can go wrong, whatever its implementation: segments longer than a wave's 64
candidates and lists of many rounds (far above 65 535 candidates in a tile), segment starts on, before and after the first and the last
lane of a wave's chunk, queries without a candidate between queries with some, every number of positions, a term at two positions, an
empty essential slice between two non-empty ones, every flavour of the tile loop, and finalist lists that fill inside a stage-B round and
across rounds.  (A tile holds at most 1024 documents, so a single segment is at most one round long; the lists here put it anywhere
across a round's boundaries.)

Every case has the route forced (`stage` = 1), runs twice on the same batch, asserts the route from last_route(), and compares with the
oracle's dense score + top-k bit for bit.  On the 9,000-doc corpus of tests/test_stage.py."""
import numpy as np
import pytest

from oracle import refimpl as O
from searcharray_amd import roaringish as rz, synth
from searcharray_amd.device_index import DeviceIndex
from tests.helpers import set_opt
from tests.test_stage import N_DOCS, VOCAB

HEAVY = 0                        # the most frequent term: ~900 postings in every 1024-doc tile
UNKNOWN = 4000                   # not in the vocabulary


@pytest.fixture(scope="module")
def corpus():
    t, d, p, lens = synth.corpus_triples(N_DOCS, VOCAB, 14, seed=31)
    words, wt = rz.encode_sorted(t, d, p)
    orc = O.OracleIndex.from_triples(t, d, p, N_DOCS, doc_lens=lens)
    docs_of = [np.unique(d[t == x]).astype(np.int64) for x in range(VOCAB)]
    return words, rz.term_offsets(wt, VOCAB), lens, orc, docs_of


_dense = {}


def dense_of(corpus, q):
    """the oracle's dense score of a query, computed once per query and shared by the cases"""
    key = tuple(int(x) for x in q)
    if key not in _dense:
        _dense[key] = corpus[3].score_terms_sum([x for x in key if 0 <= x < VOCAB])
        _dense[key].setflags(write=False)
    return _dense[key]


def check(api, corpus, queries, k, mask=None):
    words, off, lens = corpus[:3]
    set_opt("stage", 1)
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    bt = dev.batch(np.asarray(queries), k=k)
    if mask is not None:
        f = dev.doc_filter(mask=mask)
        bt.set_filter(f)
        f.close()
    for _ in range(2):                                   # (a second run on the state the first one left)
        bt.run()
    assert bt.last_route() == "staged"
    scores, docs = bt.fetch()
    bt.close()
    dev.close()
    for qi, q in enumerate(queries):
        dense = dense_of(corpus, q)
        ws, wd = O.topk(dense if mask is None else np.where(mask, dense, np.float32(0)), k)
        n = int((ws > 0).sum())
        assert np.array_equal(scores[qi, :n], ws[:n]), f"q{qi} {q} scores"
        assert np.array_equal(docs[qi, :n], wd[:n]), f"q{qi} {q} docs"
    return scores, docs


def tiles_where_essential(corpus, term, k, docs=1024):
    """tiles in which a one-term query's term is essential whatever the bound has risen to: those that hold one of its k best documents (the
    tile's bound is at least that document's score, and the query's bound never exceeds the k-th best score)"""
    _, wd = O.topk(dense_of(corpus, [term]), k)
    return np.unique(wd.astype(np.int64) // docs)


@pytest.fixture(scope="module")
def rare(corpus):
    """a term with a directory row and exactly one posting in some 1024-doc tile"""
    docs_of = corpus[4]
    for x in range(VOCAB - 1, 0, -1):
        per_tile = np.bincount(docs_of[x] // 1024, minlength=9)
        if len(docs_of[x]) >= 32 and per_tile.min() >= 1 and (per_tile == 1).sum() >= 1:
            return x
    raise AssertionError("no such term in the corpus")


# ---- a segment longer than a wave's 64 candidates; lists of many rounds
@pytest.mark.parametrize("shared_by", [1, 3, 256])
def test_long_segments_and_many_rounds(api, corpus, shared_by):
    """the most frequent term, staged and essential, shared by 1 / 3 / 256 one-term queries: segments of ~900 candidates (15 chunks), lists of
    ~900 / ~2,700 / ~230,000 candidates per tile -- one round, three rounds with segments across their boundaries, and 225 rounds.  (k = 3:
    the term is essential in the two or three tiles that hold its best documents; elsewhere the lists are empty.)"""
    set_opt("stage_probe", 0)
    set_opt("stage_docs", 1024)
    k = 3
    per_tile = np.bincount(corpus[4][HEAVY] // 1024, minlength=9)
    ess = tiles_where_essential(corpus, HEAVY, k)
    assert len(ess) >= 2 and per_tile[ess].min() > 64 and shared_by * per_tile[ess].max() > (65535 if shared_by == 256 else 1024 * (shared_by - 1))
    check(api, corpus, [[HEAVY]] * shared_by, k)


# ---- segment starts on, before and after lane 0 and lane 63 of a chunk
@pytest.mark.parametrize("p", [0, 1, 31, 32, 33, 63, 64, 65])
def test_segment_starts_around_chunk_boundaries(api, corpus, rare, p):
    """three queries on the frequent term behind p queries on a rare one with (in some tile, exactly) one candidate each: the long segments
    start at candidate p (lane p of chunk 0, or lane p - 64 of chunk 1), the short ones before them on consecutive lanes.  k = 40: every
    posting of the rare term is a candidate, and the frequent term is essential in most tiles."""
    set_opt("stage_probe", 0)
    set_opt("stage_docs", 1024)
    k = 40
    docs_of = corpus[4]
    assert len(docs_of[rare]) <= 64                      # (with k = 40 .. 64 of them wanted, hardly any posting of the rare term falls below the bound)
    ess = tiles_where_essential(corpus, HEAVY, k)
    one = np.flatnonzero(np.bincount(docs_of[rare] // 1024, minlength=9) == 1)
    assert len(ess) >= 3 and len(np.intersect1d(ess, one)) >= 1
    check(api, corpus, [[rare]] * p + [[HEAVY]] * 3, k)


# ---- queries without a candidate between queries with some
def test_holes_between_queries(api, corpus, rare):
    """256 queries of which every 7th has known terms -- the others hold unknown terms only, and most tiles of 128 docs hold no posting of
    the rare terms of those that do; and a set whose first and last queries are empty"""
    set_opt("stage_probe", 0)
    set_opt("stage_docs", 128)
    queries = [[UNKNOWN + i, UNKNOWN] for i in range(256)]
    for i in range(0, 256, 7):
        queries[i] = [VOCAB - 1 - (i % 40), 3 + (i % 5)]
    check(api, corpus, queries, 10)
    check(api, corpus, [[UNKNOWN, UNKNOWN + 1], [HEAVY, rare], [UNKNOWN, rare], [rare, UNKNOWN], [3, 5], [UNKNOWN + 2, UNKNOWN]], 10)


# ---- every number of positions; a term at two positions; an empty essential slice between two non-empty ones
@pytest.mark.parametrize("T", [1, 3, 4, 5, 8])
def test_positions(api, corpus, T):
    """T = 1, 3, 4 run the <4, ...> instances, 5 and 8 the <8, ...> ones.  Rare terms in 128-doc tiles with k = 50: every term is essential, and
    most tiles hold postings of some of a query's terms only -- empty essential slices at the start, in the middle and at the end of the
    positions; queries with a term twice; queries of frequent terms (long segments at several positions)."""
    set_opt("stage_probe", 0)
    set_opt("stage_docs", 128)
    rng = np.random.default_rng(500 + T)
    docs_of = corpus[4]
    queries = rng.integers(VOCAB - 60, VOCAB, (24, T))
    queries[1::8, 0] = rng.integers(0, 4, 3)             # (a frequent term among the rare ones)
    if T >= 3:
        queries[2::8, 2] = queries[2::8, 0]              # (the same term at two positions)
        queries[3::8, 1] = UNKNOWN                       # (a position without a term between two with one)
        # precondition on the inputs: some query has a tile with postings of its first and third term and none of its second
        def tiles_of(x):
            return np.unique(docs_of[int(x)] // 128) if 0 <= x < VOCAB else np.empty(0, np.int64)
        assert any(len(np.setdiff1d(np.intersect1d(tiles_of(r[0]), tiles_of(r[2])), tiles_of(r[1]))) > 0 for r in queries)
    check(api, corpus, queries, 50)
    check(api, corpus, np.asarray([[i % 3, 3 + i % 4, 1, 20 + i, 0, 7, 2, 9][:T] for i in range(12)]), 3)


# ---- every flavour of the tile loop
def mixed_set(rare):
    """long segments, one-candidate segments around them, queries without candidates, four positions"""
    q = [[rare, UNKNOWN, UNKNOWN, UNKNOWN]] * 5 + [[HEAVY, UNKNOWN, UNKNOWN, UNKNOWN]] * 3 + [[UNKNOWN] * 4] * 3
    q += [[1, VOCAB - 1 - i, 30 + i, HEAVY] for i in range(12)] + [[rare, 2, rare, UNKNOWN], [UNKNOWN, 1, 2, 3]]
    return q


@pytest.mark.parametrize("cw", [None, 1])
@pytest.mark.parametrize("docs", [64, 1024])
@pytest.mark.parametrize("pipe", [0, 1])
def test_every_loop_flavour(api, corpus, rare, pipe, docs, cw):
    """pipelined and not, tiles of 64 and 1024 docs, co-walking (the default) and private ranges"""
    set_opt("stage_probe", 0)
    set_opt("stage_pipe", pipe)
    set_opt("stage_docs", docs)
    if cw is not None:
        set_opt("stage_cw", cw)
    check(api, corpus, mixed_set(rare), 40)


@pytest.mark.parametrize("pipe", [0, 1])
def test_filter_with_tiles_nobody_is_eligible_in(api, corpus, rare, pipe):
    """the FILT instances: every second 64-doc tile has no eligible document, the others every third document"""
    set_opt("stage_pipe", pipe)
    set_opt("stage_docs", 64)
    set_opt("stage_wgs", 2)
    doc = np.arange(N_DOCS)
    mask = ((doc // 64) % 2 == 0) & (doc % 3 != 1)
    check(api, corpus, mixed_set(rare), 40, mask=mask)


# ---- the finalist list fills inside one stage-B round, and across rounds
@pytest.mark.parametrize("shape", ["inside_a_round", "across_rounds"])
def test_finalist_list_fills(api, corpus, shape):
    """small k, everything staged.  inside_a_round: a filter drops the starting bounds, so in a workgroup's first tile every candidate of the 24
    all-frequent queries survives both stages -- a round of 512 survivors meets a list of 384 entries.  across_rounds: 256 queries whose few
    finalists per tile add up over the rounds and tiles of a workgroup."""
    set_opt("stage_probe", 0)
    set_opt("stage_docs", 256)
    rng = np.random.default_rng(9)
    if shape == "inside_a_round":
        queries = np.stack([rng.integers(0, 3, 24), rng.integers(3, 6, 24), rng.integers(6, 12, 24), rng.integers(12, 20, 24)], axis=1)
        check(api, corpus, queries, 3, mask=np.arange(N_DOCS) % 5 != 0)
    else:
        queries = np.stack([rng.integers(0, 4, 256), rng.integers(4, 40, 256), rng.integers(40, VOCAB, 256), rng.integers(0, VOCAB, 256)], axis=1)
        check(api, corpus, queries, 3)
