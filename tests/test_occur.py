"""Required and prohibited terms (+tok / -tok; Lucene's SHOULD / MUST / MUST_NOT) for BM25 top-k batches (sa_batch_set_occur).

Semantics under test, for a query with slots t_0 .. t_{T-1}, classes occ_j in {should, must, must_not} and a per-query integer m:

    per   = [orc.score(t_j) for j in range(T)]          # float32; padding / unknown terms score 0 everywhere
    match = [s > 0 for s in per]                        # the one definition of "slot j matches doc d" (as minimum-should-match)
    dense = np.sum([zeros if occ_j == must_not else per_j for j], axis=0)      # slot order; a prohibited slot adds nothing
    ok    = all(match_j, must j) & ~any(match_j, must_not j) & (sum(match_j, should j) >= m)
    dense[~ok] = 0
    O.topk(dense, k)

bit for bit (scores and doc ids of the used slots, unused slots score 0 / doc 2**64-1).  Such a batch runs on the per-query tile
kernels' occur instantiations, whatever route the options force, and without starting bounds.  The patterns are shown, from the oracle
alone, to leave hits and to differ from the plain disjunction."""
import numpy as np
import pytest

from oracle import refimpl as O
from searcharray_amd import _lib
from searcharray_amd._lib import SearchArrayHipError
from searcharray_amd.device_index import DeviceIndex
from searcharray_amd.postings import SearchArray
from searcharray_amd.sharded import ShardedIndex
from searcharray_amd.solr import split_occur
from tests.test_abi import HEADER, declared_functions
from tests.test_min_match import NO_DOC, VARIANTS, band, check, head_queries, term_score
from tests.test_min_match import corpus  # noqa: F401  (the module's fixture: synth.corpus_triples(9000, 400, 14, seed=31))
from tests.test_sharded import n_devices

N_DOCS, VOCAB = 9000, 400
UNSUPPORTED = r"\(-5\)"                                       # SA_ERR_UNSUPPORTED in the error text
S, MUST, NOT = 0, 1, 2
PATTERNS = ("not0", "notlast", "must0", "mustlast", "mix", "mix_m", "allmust", "two_not")
BAND_PATTERNS = ("not0", "must0", "mustlast", "mix", "two_not")


def pattern(name, T):
    """(classes of the T slots, m)"""
    occ, m = [S] * T, 0
    if name == "not0":
        occ[0] = NOT
    elif name == "notlast":
        occ[-1] = NOT
    elif name == "must0":
        occ[0] = MUST
    elif name == "mustlast":
        occ[-1] = MUST
    elif name == "mix":
        occ[0], occ[1] = MUST, NOT
    elif name == "mix_m":
        occ[1], occ[2] = MUST, NOT
        m = 1 if T == 3 else 2
    elif name == "allmust":
        occ = [MUST] * T
    elif name == "two_not":
        occ[0], occ[2] = NOT, NOT
    else:
        raise KeyError(name)
    return occ, m


def occ_of(name, T, n=40):
    occ, m = pattern(name, T)
    return np.tile(np.asarray(occ, dtype=np.uint8), (n, 1)), [m] * n


# the oracle, computed once per (query set, classes, m, k, mask) and shared by every test of the module (never modified)
_wants = {}


def dense_of(orc, q, occ, m):
    """the formula of the module's docstring for one query"""
    per = [term_score(orc, int(t)) for t in q]
    zeros = np.zeros(N_DOCS, dtype=np.float32)
    dense = np.sum([zeros if c == NOT else s for s, c in zip(per, occ)], axis=0)
    assert dense.dtype == np.float32
    ok = np.ones(N_DOCS, dtype=bool)
    n_should = np.zeros(N_DOCS, dtype=np.int64)
    for s, c in zip(per, occ):
        if c == MUST:
            ok &= s > 0
        elif c == NOT:
            ok &= ~(s > 0)
        else:
            n_should += s > 0
    ok &= n_should >= m
    dense[~ok] = 0
    return dense


def want_of(orc, queries, occ, ms, k, mask=None):
    queries, occ = np.asarray(queries), np.asarray(occ)
    ms = np.broadcast_to(np.asarray(ms, dtype=np.int64), (len(queries),))
    key = (queries.tobytes(), queries.shape, occ.tobytes(), ms.tobytes(), k, None if mask is None else mask.tobytes())
    if key not in _wants:
        out = []
        for q, o, m in zip(queries, occ, ms):
            d = dense_of(orc, q, o, int(m))
            if mask is not None:
                d[~mask] = 0
            out.append(O.topk(d, k))
        _wants[key] = out
    return _wants[key]


def hits_and_differing(orc, queries, occ, ms, k):
    want, plain = want_of(orc, queries, occ, ms, k), want_of(orc, queries, np.zeros_like(occ), 0, k)
    hits = sum(int((ws > 0).any()) for ws, _ in want)
    differ = sum(not (np.array_equal(ws, us) and np.array_equal(wd[ws > 0], ud[us > 0])) for (ws, wd), (us, ud) in zip(want, plain))
    return hits, differ


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 1. every kernel variant x tile size
def cells():
    """(T, k, pattern, query set): heads at (3, 3), (4, 50), (5, 50) -- a second group of four phases with one phase --, (8, 1000) x
    every pattern; band queries at k = 50 x the patterns that leave them hits"""
    out = [(T, k, name, "head") for T, k in ((3, 3), (4, 50), (5, 50), (8, 1000)) for name in PATTERNS]
    out += [(T, 50, name, "band") for T in (4, 8) for name in BAND_PATTERNS]
    return out


def cells_for(on_emu, tile, variant):
    """all cells on the GPU; the host-emulated kernels take every third cell per (tile size, variant), shifted with the variant and the
    tile size: 42 cells, 14 of them per case, so every cell -- and with it every pattern -- is taken by two variants at every tile
    size"""
    all_cells = cells()
    if not on_emu:
        return all_cells
    shift = list(VARIANTS).index(variant) + [1024, 2048, 8192].index(tile)
    return all_cells[shift % 3::3]


def test_the_emulator_subsets_cover_every_cell():
    for tile in (1024, 2048, 8192):
        taken = [c for v in VARIANTS for c in cells_for(True, tile, v)]
        assert all(taken.count(c) >= 2 for c in cells()), tile
    assert len(cells()) == 42


@pytest.mark.parametrize("tile", [1024, 2048, 8192])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_kernel_variant_applies_the_classes(api, corpus, on_emu, variant, tile):
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=tile, api=api)
    open_bt = {}
    for T, k, name, kind in cells_for(on_emu, tile, variant):
        what = f"{variant} tile {tile} T {T} k {k} {name} {kind}"
        queries = head_queries(T) if kind == "head" else band(T)
        occ, ms = occ_of(name, T)
        if (T, k, kind) not in open_bt:
            open_bt[(T, k, kind)] = dev.batch(queries, k=k, opts=VARIANTS[variant])
        bt = open_bt[(T, k, kind)]
        bt.set_occur(occ)
        bt.set_min_match(ms)
        for _ in range(2):                                       # the second run on the state the first one left
            bt.run()
        assert bt.last_route() == "exhaustive", f"{what}: route {bt.last_route()}"
        assert not bt.seeds().any(), f"{what}: such a run must not start from the corpus-wide bounds"
        check(bt.fetch(), want_of(orc, queries, occ, ms, k), what)
    for bt in open_bt.values():
        bt.close()
    dev.close()


# ---- 2. not vacuous: from the oracle alone
def test_the_patterns_cannot_pass_by_ignoring_the_classes(corpus):
    orc = corpus[3]
    for T in (4, 5, 8):
        for name in PATTERNS:
            occ, ms = occ_of(name, T)
            hits, differ = hits_and_differing(orc, head_queries(T), occ, ms, 50)
            assert hits >= 20 and differ >= 30, f"heads T {T} {name}: hits {hits}, differing {differ} of 40"
    for T in (4, 8):
        for name in BAND_PATTERNS:
            occ, ms = occ_of(name, T)
            hits, differ = hits_and_differing(orc, band(T), occ, ms, 50)
            assert hits >= 30 and differ >= 30, f"band T {T} {name}: hits {hits}, differing {differ} of 40"


# ---- 3. cross-checks against existing behaviour
def test_allmust_is_min_match_T_and_all_should_is_the_plain_batch(api, corpus):
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    queries = head_queries(4)
    bt = dev.batch(queries, k=50)
    bt.run()
    plain, route, seeds = bt.fetch(), bt.last_route(), bt.seeds()
    bt.set_min_match([4] * 40)
    bt.run()
    by_mm = bt.fetch()
    bt.set_min_match(None)
    bt.set_occur(np.full((40, 4), MUST))
    bt.run()
    assert same(bt.fetch(), by_mm), "allmust vs min_match = T"
    assert not same(by_mm, plain)
    # all slots should, then no classes: the batch as it was -- same route, same starting bounds, same bits
    for values in (np.zeros((40, 4), dtype=np.int64), None):
        bt.set_occur(np.full((40, 4), NOT))
        bt.set_occur(values)
        bt.run()
        assert same(bt.fetch(), plain), f"occur {values is not None}"
        assert bt.last_route() == route and np.array_equal(bt.seeds(), seeds)
    bt.close()
    bt = dev.batch(queries, k=50, occur=np.zeros((40, 4), dtype=np.uint8))
    bt.run()
    assert same(bt.fetch(), plain) and bt.last_route() == route and np.array_equal(bt.seeds(), seeds)
    bt.close()
    dev.close()


@pytest.mark.parametrize("j", [0, 2])
def test_must_and_must_not_are_term_filters(api, corpus, j):
    """a set where every query has the same term in slot j: must = the plain batch inside term_filter(t_j); must_not = the batch of
    the other slots outside it"""
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=2048, api=api)
    tj = 3
    queries = np.stack([q for q in head_queries(4, n=80) if tj not in q][:40])
    queries[:, j] = tj
    rest = np.delete(queries, j, axis=1)
    f = dev.term_filter(tj)
    for cls, ref_q, ref_f in ((MUST, queries, f), (NOT, rest, ~f)):
        ref = dev.batch(ref_q, k=50, filter=ref_f)
        ref.run()
        want = ref.fetch()
        ref.close()
        occ = np.zeros((40, 4), dtype=np.uint8)
        occ[:, j] = cls
        bt = dev.batch(queries, k=50, occur=occ)
        bt.run()
        got = bt.fetch()
        assert same(got, want), f"class {cls} on slot {j}"
        assert (got[0] > 0).any()
        check(got, want_of(orc, queries, occ, 0, 50), f"class {cls} on slot {j}: oracle")
        bt.close()
    dev.close()


# ---- 4. edges
@pytest.mark.parametrize("tile", [1024, 4096])
def test_edges(api, corpus, tile):
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=tile, api=api)
    q4 = head_queries(4)
    # an unknown id under must: nothing for those queries, the others as the oracle says
    qu = q4.copy()
    qu[::2, 2] = VOCAB
    occ = np.zeros((40, 4), dtype=np.uint8)
    occ[:, 2] = MUST
    bt = dev.batch(qu, k=10, occur=occ)
    bt.run()
    s, d = bt.fetch()
    assert not s[::2].any() and (d[::2] == NO_DOC).all() and s[1::2].any()
    check((s, d), want_of(orc, qu, occ, 0, 10), "unknown term under must")
    # an unknown id under must_not: the same as without the slot
    occ[:, 2] = NOT
    bt.set_occur(occ)
    bt.run()
    got = bt.fetch()
    check(got, want_of(orc, qu, occ, 0, 10), "unknown term under must_not")
    ref = dev.batch(np.delete(qu[::2], 2, axis=1), k=10)
    ref.run()
    rs, rd = ref.fetch()
    ref.close()
    assert np.array_equal(got[0][::2], rs) and np.array_equal(got[1][::2], rd)
    # only must_not slots: nothing
    bt.set_occur(np.full((40, 4), NOT))
    bt.run()
    s, d = bt.fetch()
    assert not s.any() and (d == NO_DOC).all()
    # m above the number of should slots: nothing
    occ = np.zeros((40, 4), dtype=np.uint8)
    occ[:, 0] = MUST
    bt.reset(q4)
    bt.set_occur(occ)
    bt.set_min_match([4] * 40)
    bt.run()
    s, d = bt.fetch()
    assert not s.any() and (d == NO_DOC).all()
    check((s, d), want_of(orc, q4, occ, 4, 10), "m above the should slots")
    bt.set_min_match([3] * 40)                                   # ... and all of them: the conjunction
    bt.run()
    got = bt.fetch()
    check(got, want_of(orc, q4, occ, 3, 10), "m = the should slots")
    assert got[0].any()
    bt.close()
    # [a, a, b] with [+, s, -]: the docs with a and without b, scored 2 x a
    qd = np.asarray([[5, 5, 390], [9, 9, 399], [0, 0, 1], [1, 1, 0]])
    occ = np.tile(np.asarray([MUST, S, NOT], dtype=np.uint8), (4, 1))
    bt = dev.batch(qd, k=50, occur=occ)
    bt.run()
    want = want_of(orc, qd, occ, 0, 50)
    check(bt.fetch(), want, "[a, a, b] with [+, s, -]")
    a, b = term_score(orc, 0), term_score(orc, 1)
    top = want[2][1][want[2][0] > 0].astype(np.int64)
    assert len(top) and (a[top] > 0).all() and not (b[top] > 0).any() and np.array_equal(want[2][0][want[2][0] > 0], (a + a)[top])
    bt.close()
    # T = 1 with each class
    q1 = np.asarray([[0], [0], [0], [VOCAB], [VOCAB], [350]])
    occ = np.asarray([[S], [MUST], [NOT], [MUST], [NOT], [MUST]], dtype=np.uint8)
    bt = dev.batch(q1, k=10, occur=occ)
    bt.run()
    got = bt.fetch()
    check(got, want_of(orc, q1, occ, 0, 10), "T = 1")
    assert same((got[0][:1], got[1][:1]), (got[0][1:2], got[1][1:2])) and got[0][0].any() and got[0][5].any()
    assert not got[0][2:5].any()
    bt.close()
    # m = 0 with a must slot and no should match: the doc is kept (term 399 is rare: most docs of term 0 lack it)
    q2 = np.asarray([[0, 399], [399, 0]])
    occ = np.asarray([[MUST, S], [S, MUST]], dtype=np.uint8)
    bt = dev.batch(q2, k=50, occur=occ)
    bt.run()
    want = want_of(orc, q2, occ, 0, 50)
    check(bt.fetch(), want, "m = 0 beside a must slot")
    top = want[0][1][want[0][0] > 0].astype(np.int64)
    assert (~(term_score(orc, 399)[top] > 0)).any(), "a doc without a should match is in the top-k"
    bt.set_min_match([1, 1])                                     # ... and with m = 1 it is not
    bt.run()
    want = want_of(orc, q2, occ, 1, 50)
    check(bt.fetch(), want, "m = 1 beside a must slot")
    top = want[0][1][want[0][0] > 0].astype(np.int64)
    assert (term_score(orc, 399)[top] > 0).all()
    bt.close()
    dev.close()


# ---- 5. mixed rows
def test_mixed_rows_and_a_reordered_batch(api, corpus):
    """a pattern and an m of its own per row, over a batch whose device rows are not in caller order; the classes stay with the caller's
    rows across reset"""
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=2048, api=api)
    rng = np.random.default_rng(19)
    queries = np.stack([rng.choice(16, 4, replace=False) for _ in range(200)])
    occ = rng.choice(np.asarray([S, S, MUST, NOT], dtype=np.uint8), size=(200, 4))
    ms = rng.integers(0, 4, 200)
    assert len({bytes(o) for o in occ}) > 40 and len(set(ms)) == 4
    bt = dev.batch(queries, k=20, occur=occ, min_match=ms)
    rows = bt.row_order()
    assert sorted(rows) == list(range(200)) and not np.array_equal(rows, np.arange(200)), "the device rows are not in caller order"
    bt.run()
    got = bt.fetch()
    want = want_of(orc, queries, occ, ms, 20)
    check(got, want, "mixed rows")
    assert 40 <= sum(int((ws > 0).any()) for ws, _ in want) < 200
    # new queries: the classes and the values stay with the caller's rows
    other = np.stack([rng.choice(16, 4, replace=False) for _ in range(200)])
    bt.reset(other)
    bt.run()
    check(bt.fetch(), want_of(orc, other, occ, ms, 20), "mixed rows, after reset")
    # new classes on the loaded set
    occ2 = rng.choice(np.asarray([S, MUST, NOT], dtype=np.uint8), size=(200, 4))
    bt.set_occur(occ2)
    bt.run()
    check(bt.fetch(), want_of(orc, other, occ2, ms, 20), "mixed rows, new classes")
    bt.close()
    dev.close()


def test_classes_persist_across_step(api, corpus):
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    dev.set_idf_table(dev.idfs(np.arange(VOCAB)))
    rng = np.random.default_rng(29)
    sets = [np.stack([rng.choice(16, 4, replace=False) for _ in range(40)]) for _ in range(3)]
    occ = rng.choice(np.asarray([S, S, MUST, NOT], dtype=np.uint8), size=(40, 4))
    bt = dev.batch(sets[0], k=10)
    bt.run(sync=False)                                           # a run nobody has fetched keeps the state it ran with
    bt.set_occur(occ)
    check(bt.fetch(), want_of(orc, sets[0], np.zeros_like(occ), 0, 10), "unfetched run, then set_occur")
    bt.step(np.ascontiguousarray(sets[1], dtype=np.uint32))
    check(bt.fetch(), want_of(orc, sets[1], occ, 0, 10), "step")
    bt.set_occur(None)
    bt.step(np.ascontiguousarray(sets[2], dtype=np.uint32))
    check(bt.fetch(), want_of(orc, sets[2], np.zeros_like(occ), 0, 10), "step after set_occur(None)")
    bt.close()
    dev.close()


# ---- 6. with a filter: a doc must pass both tests
def test_with_a_filter(api, corpus):
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    queries = head_queries(4)
    random10 = np.random.default_rng(6).random(N_DOCS) < 0.1
    a_range = np.zeros(N_DOCS, dtype=bool)
    a_range[2048:5500] = True                                    # (whole tiles empty on either side)
    for fname, mask in (("10%", random10), ("range", a_range)):
        f = dev.doc_filter(mask=mask)
        for name in ("mix", "two_not", "mix_m"):
            occ, ms = occ_of(name, 4)
            bt = dev.batch(queries, k=50, filter=f, occur=occ, min_match=ms)
            bt.run()
            want = want_of(orc, queries, occ, ms, 50, mask)
            check(bt.fetch(), want, f"filter {fname} {name}")
            assert sum(int((ws > 0).any()) for ws, _ in want) >= 20
            bt.set_filter(None)                                  # ... and each of the two can go on its own
            bt.run()
            check(bt.fetch(), want_of(orc, queries, occ, ms, 50), f"filter {fname} {name}: filter cleared")
            bt.set_filter(f)
            bt.set_occur(None)
            bt.run()
            check(bt.fetch(), want_of(orc, queries, np.zeros_like(occ), ms, 50, mask), f"filter {fname} {name}: classes cleared")
            bt.close()
    dev.close()


# ---- 7. sharded
def test_sharded_equals_the_single_index(api, corpus):
    words, off, lens, orc = corpus
    queries = head_queries(4)
    rng = np.random.default_rng(11)
    occ = rng.choice(np.asarray([S, S, MUST, NOT], dtype=np.uint8), size=(40, 4))
    ms = rng.integers(0, 3, 40)
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    bt = dev.batch(queries, k=10, occur=occ, min_match=ms)
    bt.run()
    single = bt.fetch()
    bt.close()
    dev.close()
    check(single, want_of(orc, queries, occ, ms, 10), "single index")
    for G in sorted({1, n_devices(api, 2)}):
        sh = ShardedIndex(words, off, lens, devices=list(range(G)), tile_docs=1024, api=api)
        sb = sh.batch(queries, k=10, occur=occ, min_match=ms)
        sb.run()
        assert same(sb.fetch(), single), f"{G} shard(s) vs the single index"
        occ2, _ = occ_of("mix", 4)
        sb.set_occur(occ2)
        sb.run()
        check(sb.fetch(), want_of(orc, queries, occ2, ms, 10), f"{G} shard(s), set_occur")
        sb.set_occur(None)
        sb.set_min_match(None)
        sb.run()
        check(sb.fetch(), want_of(orc, queries, np.zeros_like(occ), 0, 10), f"{G} shard(s), cleared")
        with pytest.raises(ValueError):
            sb.set_occur(occ[:39])
        sb.close()
        sh.close()


# ---- 8. SearchArray.search(occur=)
def test_split_occur():
    tok = str.split
    assert split_occur("+a b -c", tok) == (["a", "b", "c"], [1, 0, 2])
    assert split_occur("  a   -b ", tok) == (["a", "b"], [0, 2])
    assert split_occur("+a.b x", lambda s: s.split(".")) == (["a", "b", "x"], [1, 1, 0])
    assert split_occur(["+a", "b", "-c", "-", "+"], tok) == (["a", "b", "c", "-", "+"], [1, 0, 2, 0, 0])
    assert split_occur("", tok) == ([], [])
    with pytest.raises(TypeError):
        split_occur(["a", 3], tok)


def test_search_with_occur(default_api):
    rng = np.random.default_rng(3)
    vocab = [f"w{i}" for i in range(30)]
    p = 1.0 / np.arange(1, 31)
    p /= p.sum()
    docs = [" ".join(rng.choice(vocab, size=max(1, rng.poisson(12)), p=p)) for _ in range(700)]
    arr = SearchArray.index(docs)
    K = 700                                                      # every row: a test shows in the number of hits
    toks = [["w0", "w7", "w20"], ["w3", "w29", "w1", "w2"], ["w1"], ["nope", "w2", "w0"], ["w5", "w5", "w11"], ["w0", "w1", "w2", "w3", "w4"]]
    occur = [["+", "", "-"], ["must_not", "should", 1, 0], None, ["-", "must", ""], [1, 0, 2], ["", "+", "-", "", ""]]
    classes = [[1, 0, 2], [2, 0, 1, 0], [0], [2, 1, 0], [1, 0, 2], [0, 1, 2, 0, 0]]
    plain = arr.search(toks, k=K)

    def check_search(got, ms, what, mask=None):
        scores, ids = got
        for i, (q, cl) in enumerate(zip(toks, classes)):
            per = [arr.score(t) for t in q]
            dense = np.sum([np.zeros_like(s) if c == NOT else s for s, c in zip(per, cl)], axis=0)
            ok = np.ones(len(dense), dtype=bool)
            n_should = np.zeros(len(dense), dtype=np.int64)
            for s, c in zip(per, cl):
                if c == MUST:
                    ok &= s > 0
                elif c == NOT:
                    ok &= ~(s > 0)
                else:
                    n_should += s > 0
            dense[~(ok & (n_should >= ms[i]))] = 0
            if mask is not None:
                dense[~mask] = 0
            order = np.lexsort((np.arange(len(dense)), -dense))[:K]
            n = int((dense[order] > 0).sum())
            assert np.array_equal(ids[i, :n], order[:n].astype(np.uint64)) and np.array_equal(scores[i, :n], dense[order][:n]), f"{what} q{i}"
            assert not scores[i, n:].any() and (ids[i, n:] == NO_DOC).all(), f"{what} q{i} unused slots"

    got = arr.search(toks, k=K, occur=occur)
    check_search(got, [0] * 6, "occur lists")
    assert (got[0] > 0).sum() < (plain[0] > 0).sum() and all(got[0][i].any() for i in (0, 1, 2, 3, 4, 5))
    # the same from the prefixes: token lists and strings
    pre_lists = [["+w0", "w7", "-w20"], ["-w3", "w29", "+w1", "w2"], ["w1"], ["-nope", "+w2", "w0"], ["+w5", "w5", "-w11"], ["w0", "+w1", "-w2", "w3", "w4"]]
    pre_strings = [" ".join(q) for q in pre_lists]
    for name, qs in (("token lists", pre_lists), ("strings", pre_strings), ("both", pre_lists[:3] + pre_strings[3:])):
        assert same(arr.search(qs, k=K, occur="prefix"), got), f"prefix, {name}"
    split = [split_occur(q, arr.tokenizer) for q in pre_strings]
    assert [s[0] for s in split] == toks and [s[1] for s in split] == classes
    assert same(arr.search([s[0] for s in split], k=K, occur=[s[1] for s in split]), got), "parsed once by the caller"
    # without any sign, and with all-should lists: the plain search
    assert same(arr.search(toks, k=K, occur="prefix"), plain) and same(arr.search(toks, k=K, occur=[None] * 6), plain)
    assert same(arr.search(toks, k=K, occur=[[0] * len(q) for q in toks]), plain)
    # mm resolves against the should tokens only: "2" is 1 where a query has one should token, 0 where it has none
    n_should = [sum(c == 0 for c in cl) for cl in classes]
    assert n_should == [1, 2, 1, 1, 1, 3]
    check_search(arr.search(toks, k=K, occur=occur, mm="2"), [min(2, n) for n in n_should], "mm 2")
    check_search(arr.search(toks, k=K, occur=occur, mm=1), [1] * 6, "mm 1")
    assert (arr.search(toks, k=K, occur=occur, mm=1)[0] > 0).sum() < (got[0] > 0).sum(), "beside a must token m = 1 is a test"
    check_search(arr.search(toks, k=K, occur=occur, q_op="AND"), n_should, "q_op AND")
    mask = np.random.default_rng(4).random(700) < 0.5
    check_search(arr.search(toks, k=K, occur=occur, filter=mask), [0] * 6, "occur and a filter", mask=mask)
    assert same(arr.search(toks, k=K, occur=occur, devices=[0]), got), "devices=[0]"
    # errors, before anything is launched
    for bad in (occur[:5], occur + [None], [["+", ""]] + occur[1:], [["+", "", "-", ""]] + occur[1:], [["+", "", "not"]] + occur[1:],
                [["+", "", 3]] + occur[1:], [["+", "", True]] + occur[1:], ["+s-"] + occur[1:], "prefixes", 1, [1] * 6):
        with pytest.raises(ValueError):
            arr.search(toks, k=K, occur=bad)
    with pytest.raises(TypeError):
        arr.search_phrases([["w0", "w1"]], k=K, occur=[["+", ""]])
    with pytest.raises(ValueError, match="slice"):
        arr[:100].search(toks, k=10, occur=occur)


def test_error_paths(api, corpus):
    words, off, lens, orc = corpus
    dev = DeviceIndex(words, off, lens, tile_docs=1024, api=api)
    queries = head_queries(4)
    occ, _ = occ_of("mix", 4)
    pb = dev.phrase_batch([[0, 1], [2, 0]], k=5)
    with pytest.raises(SearchArrayHipError, match=UNSUPPORTED + ".*phrase"):     # (the C call itself: a phrase batch handle)
        api.call("sa_batch_set_occur", pb._h, np.zeros(4, dtype=np.uint8).ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_uint8)))
    pb.close()
    bt = dev.batch(queries, k=10, opts={"no_topk": 1})
    with pytest.raises(SearchArrayHipError, match=UNSUPPORTED + ".*no_topk"):
        bt.set_occur(occ)
    bt.close()
    big = DeviceIndex(words, off, lens, tile_docs=16384, api=api)
    bt = big.batch(queries, k=10)
    with pytest.raises(SearchArrayHipError, match=UNSUPPORTED + ".*tile_docs"):
        bt.set_occur(occ)
    bt.set_occur(np.zeros((40, 4), dtype=np.uint8))              # (all should needs no counting kernel)
    bt.run()
    check(bt.fetch(), want_of(orc, queries, np.zeros_like(occ), 0, 10), "16384-doc tiles, all should")
    bt.close()
    big.close()
    # the Python layer: wrong shapes, classes out of range, not integers -- before a launch
    bt = dev.batch(queries, k=10)
    for bad in (occ[:39], occ[:, :3], occ.reshape(-1), np.full((40, 4), 3), np.full((40, 4), -1), occ.astype(np.float32), 1):
        with pytest.raises(ValueError):
            bt.set_occur(bad)
        with pytest.raises(ValueError):
            dev.batch(queries, k=10, occur=bad)
    # ... and the C call checks the classes itself
    with pytest.raises(SearchArrayHipError, match="occur classes"):
        api.call("sa_batch_set_occur", bt._h, np.full(160, 3, dtype=np.uint8).ctypes.data_as(_lib.ctypes.POINTER(_lib.ctypes.c_uint8)))
    bt.run()
    check(bt.fetch(), want_of(orc, queries, np.zeros_like(occ), 0, 10), "after the rejected calls")
    bt.close()
    dev.close()


# ---- 9. ABI
def test_the_new_calls_are_declared_and_bound():
    names = declared_functions()
    for name in ("sa_batch_set_occur", "sa_sharded_batch_set_occur"):
        assert name in names and name in _lib.PROTOTYPES
    from tests.emu import emu_api
    assert hasattr(emu_api(), "sa_batch_set_occur") and hasattr(emu_api(), "sa_sharded_batch_set_occur")
    header = open(HEADER).read()
    assert "int sa_batch_set_occur(sa_batch_t* batch, const uint8_t* occur);" in header
