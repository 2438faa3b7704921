"""The staged-tile kernel's tile loop pipelined by one tile (csrc/sa_stage.hip, template parameter PIPE; option `stage_pipe`):
pass i builds tile i + 1's layout -- slice sizes, block scan, stage offsets, chunk list -- while its own stage loads are in flight, into
the other half of a double-buffered s_off / s_tmax.  The cases are the smallest shapes at which a one-tile pipeline can go wrong:
workgroups with 0 .. 18 tiles and a partial last tile (prologue, epilogue), a tile that does not fit the stage between fitting ones,
a filter with tiles nobody is eligible in, the sets that keep the un-pipelined loop, finalist lists that fill within a tile, six and
eight terms per query.

Every case runs twice -- with `stage_pipe` = 1, pipelined where the set is eligible (one staged term per thread, every staged term with a
directory row), and with `stage_pipe` = 0 -- and both runs must equal the oracle's dense score + top-k bit for bit, hence each other.  Which loop ran is
read from the launch's own trace line.  (On a full device the 9,000-doc corpus gives a workgroup one tile at most: there the cases
check the pipelined instances' prologue; the host-emulated 4-CU device gives a workgroup up to 18.)"""
import numpy as np
import pytest

from oracle import refimpl as O
from searcharray_amd import roaringish as rz, synth
from searcharray_amd.device_index import DeviceIndex
from tests.helpers import set_opt, unset_opt
from tests.test_stage import N_DOCS, VOCAB, band_queries

CAP4 = 2304                      # SaStCap<4>::v: 8-byte cells of the LDS stage (queries of up to 4 terms)


@pytest.fixture(scope="module")
def corpus():
    t, d, p, lens = synth.corpus_triples(N_DOCS, VOCAB, 14, seed=31)
    words, wt = rz.encode_sorted(t, d, p)
    return words, rz.term_offsets(wt, VOCAB), lens, O.OracleIndex.from_triples(t, d, p, N_DOCS, doc_lens=lens), VOCAB


@pytest.fixture(scope="module")
def frequent(corpus):
    """terms with a directory row whatever the tile size: df >= max(32, tiles / 8), 141 tiles of 64 docs at most"""
    orc = corpus[3]
    f = np.asarray([t for t in range(VOCAB) if orc.docfreq(t) >= 64])
    assert len(f) >= 40
    return f


_dense = {}


def dense_of(corpus, q):
    """the oracle's dense score of a query, computed once per (corpus, query) and shared by the cases"""
    orc, vocab = corpus[3], corpus[4]
    key = (id(orc), tuple(int(x) for x in q))
    if key not in _dense:
        _dense[key] = orc.score_terms_sum([x for x in key[1] if 0 <= x < vocab])
        _dense[key].setflags(write=False)
    return _dense[key]


def run_once(dev, queries, k, mask, want, capfd, runs):
    bt = dev.batch(np.asarray(queries), k=k)
    if mask is not None:
        f = dev.doc_filter(mask=mask)
        bt.set_filter(f)
        f.close()
    capfd.readouterr()
    for _ in range(runs):                                # (a second run on the state the first one left)
        bt.run()
    trace = capfd.readouterr().err
    assert bt.last_route() == "staged"
    scores, docs = bt.fetch()
    bt.close()
    for qi, (ws, wd) in enumerate(want):
        n = int((ws > 0).sum())
        assert np.array_equal(scores[qi, :n], ws[:n]), f"q{qi} {queries[qi]} scores"
        assert np.array_equal(docs[qi, :n], wd[:n]), f"q{qi} {queries[qi]} docs"
    return scores, docs, trace


def both(api, corpus, queries, k, capfd, pipelined=True, mask=None):
    """the set on the pipelined loop (where eligible: `pipelined`) and on the un-pipelined one: both equal the oracle, and each other"""
    words, off, lens = corpus[:3]
    want = []
    for q in queries:
        dense = dense_of(corpus, q)
        want.append(O.topk(dense if mask is None else np.where(mask, dense, np.float32(0)), k))
    set_opt("stage", 1)
    set_opt("trace", 1)
    set_opt("stage_pipe", 1)                             # (wherever eligible: the library's own rule pipelines from 256 staged terms on)
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    s1, d1, tr = run_once(dev, queries, k, mask, want, capfd, 2)
    assert ("tile loop pipelined" in tr) == pipelined and ("tile loop not pipelined" in tr) != pipelined, tr
    set_opt("stage_pipe", 0)
    s0, d0, tr = run_once(dev, queries, k, mask, want, capfd, 1)
    assert "tile loop not pipelined" in tr and "tile loop pipelined" not in tr, tr
    unset_opt("stage_pipe")
    dev.close()
    assert np.array_equal(s1, s0) and np.array_equal(d1, d0)


# ---- prologue and epilogue
@pytest.mark.parametrize("cw", [1, 2, 4])
@pytest.mark.parametrize("wgs", [8, 4, 2])
def test_few_tiles_per_workgroup(api, corpus, frequent, capfd, wgs, cw):
    """141 tiles of 64 docs (the last one of 40) over 32 / 16 / 8 workgroups of the emulated device, private ranges and co-walking groups:
    workgroups with 5 / 9 / 18 tiles, with 3 or 4 (the last XCD's, co-walked), with none, and the partial last tile"""
    set_opt("stage_docs", 64)
    set_opt("stage_wgs", wgs)
    set_opt("stage_cw", cw)
    rng = np.random.default_rng(1000 + 10 * wgs + cw)
    queries = frequent[rng.integers(0, len(frequent), (24, 4))]
    both(api, corpus, queries, 10, capfd)


# ---- a tile that does not fit the stage between tiles that do
OV_TILES, OV_TERMS, OV_BG = 24, 24, 100
OVER = sorted([t for t in range(21) if t % 3 == 1] + [21, 23])     # (workgroups of three tiles: fits / over / fits, and the last one over / fits / over)


@pytest.fixture(scope="module")
def band_corpus():
    """24 x 1024 docs: two of 100 background terms per doc everywhere (at most 2048 postings per tile), and in the docs of the OVER tiles
    every one of 24 band terms on top (24,576 postings per tile)"""
    n_docs, vocab = OV_TILES * 1024, OV_TERMS + OV_BG
    rng = np.random.default_rng(8)
    docs = np.arange(n_docs, dtype=np.int64)
    a = rng.integers(0, OV_BG, n_docs)
    b = (a + 1 + rng.integers(0, OV_BG - 1, n_docs)) % OV_BG
    band = docs[np.isin(docs // 1024, OVER)]
    t = np.concatenate([OV_TERMS + a, OV_TERMS + b, np.repeat(np.arange(OV_TERMS), len(band))])
    d = np.concatenate([docs, docs, np.tile(band, OV_TERMS)])
    p = np.concatenate([np.zeros(n_docs, np.int64), np.ones(n_docs, np.int64), np.full(OV_TERMS * len(band), 2, np.int64)])
    order = np.lexsort((p, d, t))
    t, d, p = t[order].astype(np.uint32), d[order].astype(np.uint32), p[order].astype(np.uint32)
    lens = np.bincount(d, minlength=n_docs).astype(np.float32)
    words, wt = rz.encode_sorted(t, d, p)
    return (words, rz.term_offsets(wt, vocab), lens, O.OracleIndex.from_triples(t, d, p, n_docs, doc_lens=lens), vocab), (t, d)


def test_oversize_tile_between_fitting_tiles(api, band_corpus, capfd):
    corpus, (t, d) = band_corpus
    rng = np.random.default_rng(12)
    queries = np.stack([rng.integers(0, OV_TERMS, 24), OV_TERMS + rng.integers(0, OV_BG, 24), OV_TERMS + rng.integers(0, OV_BG, 24),
                        rng.integers(0, OV_TERMS, 24)], axis=1)
    # precondition on the inputs: postings of the batch's distinct terms per 1024-doc tile, against the stage's cells
    distinct = np.unique(queries)
    per_tile = np.bincount(d[np.isin(t, distinct)].astype(np.int64) // 1024, minlength=OV_TILES)
    over = per_tile > CAP4
    assert over.sum() >= 2 and (~over).sum() >= 2 and sorted(np.flatnonzero(over)) == OVER
    assert any(over[i] and not over[i + 1] for i in range(OV_TILES - 1)) and any(not over[i] and over[i + 1] for i in range(OV_TILES - 1))
    assert per_tile[~over].max() < CAP4 and len(distinct) <= 512
    set_opt("stage_probe", 0)
    set_opt("stage_docs", 1024)
    both(api, corpus, queries, 10, capfd)


# ---- a filter with tiles nobody is eligible in
@pytest.mark.parametrize("which", ["every_second_tile", "first_and_last_of_a_workgroup"])
def test_filter_with_empty_tiles(api, corpus, frequent, capfd, which):
    set_opt("stage_docs", 64)
    set_opt("stage_wgs", 2)                              # (the emulated device: 8 workgroups, one per XCD, 18 consecutive tiles each -- the last one 15)
    set_opt("stage_cw", 1)
    n_st = (N_DOCS + 63) // 64
    tile = np.arange(N_DOCS) // 64
    if which == "every_second_tile":
        mask = tile % 2 == 0
    else:
        tpx = (n_st + 7) // 8
        edge = {x * tpx for x in range(8)} | {min(x * tpx + tpx - 1, n_st - 1) for x in range(8)}
        mask = ~np.isin(tile, sorted(edge))
    rng = np.random.default_rng(77)
    queries = frequent[rng.integers(0, len(frequent), (24, 4))]
    both(api, corpus, queries, 10, capfd, mask=mask)


# ---- the sets that keep the un-pipelined loop
@pytest.fixture(scope="module")
def rare_corpus():
    """the same 9,000 docs over 4,000 terms: most of them in fewer than 32 docs -- no directory row at any tile size"""
    vocab = 4000
    t, d, p, lens = synth.corpus_triples(N_DOCS, vocab, 14, seed=31)
    words, wt = rz.encode_sorted(t, d, p)
    return words, rz.term_offsets(wt, vocab), lens, O.OracleIndex.from_triples(t, d, p, N_DOCS, doc_lens=lens), vocab


def test_rare_term_keeps_the_unpipelined_loop(api, rare_corpus, capfd):
    """a term too rare for a directory row is walked by its owner thread: private ranges, no pipeline"""
    set_opt("stage_docs", 64)
    set_opt("stage_wgs", 8)
    orc = rare_corpus[3]
    rare = np.asarray([t for t in range(1000, 3000) if 0 < orc.docfreq(t) < 32])
    assert len(rare) >= 24
    rng = np.random.default_rng(41)
    queries = np.stack([rng.choice([0, 1, 5], 24), rng.integers(3, 60, 24), rare[:24]], axis=1)
    both(api, rare_corpus, queries, 3, capfd, pipelined=False)


@pytest.fixture(scope="module")
def wide_corpus():
    """4096 docs of 20 terms drawn from 640: every term in ~128 docs (a directory row for each at 64 tiles)"""
    n_docs, vocab, per_doc = 4096, 640, 20
    rng = np.random.default_rng(3)
    t = rng.integers(0, vocab, n_docs * per_doc)
    d = np.repeat(np.arange(n_docs), per_doc)
    p = np.tile(np.arange(per_doc), n_docs)
    order = np.lexsort((p, d, t))
    t, d, p = t[order].astype(np.uint32), d[order].astype(np.uint32), p[order].astype(np.uint32)
    lens = np.full(n_docs, per_doc, dtype=np.float32)
    words, wt = rz.encode_sorted(t, d, p)
    orc = O.OracleIndex.from_triples(t, d, p, n_docs, doc_lens=lens)
    assert min(orc.docfreq(x) for x in range(vocab)) >= 64
    return words, rz.term_offsets(wt, vocab), lens, orc, vocab


def test_two_terms_per_thread_keep_the_unpipelined_loop(api, wide_corpus, capfd):
    """640 staged terms: the two-terms-per-thread instance, which has no LDS for a second half"""
    set_opt("stage_docs", 64)
    set_opt("stage_probe", 0)
    queries = np.arange(640).reshape(160, 4)
    both(api, wide_corpus, queries, 5, capfd, pipelined=False)


def test_the_library_pipelines_from_256_staged_terms_on(api, wide_corpus, capfd):
    """option unset: 400 staged terms (all with a directory row, one per thread) are pipelined, 40 are not"""
    set_opt("stage_docs", 64)
    set_opt("stage_probe", 0)
    set_opt("stage", 1)
    set_opt("trace", 1)
    words, off, lens = wide_corpus[:3]
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    for n, pipelined in ((100, True), (10, False)):
        queries = np.arange(4 * n).reshape(n, 4)
        want = [O.topk(dense_of(wide_corpus, q), 5) for q in queries]
        _, _, tr = run_once(dev, queries, 5, None, want, capfd, 1)
        assert ("tile loop pipelined" in tr) == pipelined and ("tile loop not pipelined" in tr) != pipelined, tr
    dev.close()


# ---- finalist pressure: the list of finalists fills within a tile
@pytest.mark.parametrize("k", [1000, 3])
def test_finalist_pressure(api, corpus, frequent, capfd, k):
    """all-frequent queries (every term essential: every posting a candidate), a term repeated inside a query, unknown terms"""
    set_opt("stage_docs", 256)                           # (36 tiles: up to five per workgroup of the emulated device)
    queries = [[0, 1, 2, 3], [0, 0, 0, 5], [0, 2, 1, 1], [0, 4000, 17, 4001], [0, 4000, 4000, 4000], [5, 1, 0, 2], [4000, 0, 1, 2],
               [9, 8, 7, 6], [4000, 4001, 4002, 4003]]
    queries += [[0, int(frequent[10 + i]), int(frequent[-1 - i]), int(frequent[20 + i])] for i in range(20)]
    both(api, corpus, queries, k, capfd)


# ---- six and eight terms per query: the <8, 1, *> instances
@pytest.mark.parametrize("T", [6, 8])
def test_wide_queries(api, corpus, frequent, capfd, T):
    set_opt("stage_docs", 64)
    set_opt("stage_wgs", 2)
    rng = np.random.default_rng(60 + T)
    queries = frequent[rng.integers(0, len(frequent), (24, T))]
    both(api, corpus, queries, 10, capfd)
