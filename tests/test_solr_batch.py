"""searcharray_amd.solr.edismax_search_batch: a list of multi-field queries ranked by one fields batch (csrc/sa_fields.hip).

The yardstick is the HOST route, never the code under test: `edismax(frame, use_device=False, ...)` per query, ranked with the numpy
selection of tests/test_solr_search.py (`yardstick` / `check`: found, rows, scores with their dtype, explain), plus
`edismax_search` on the query alone.  Every comparison is exact."""
import json
import threading

import numpy as np
import pandas as pd
import pytest

from searcharray_amd import SearchArray, solr, synth
from searcharray_amd.device_index import NO_DOC
from searcharray_amd.similarity import bm25_similarity
from searcharray_amd.solr import edismax, edismax_search, edismax_search_batch, parse_query_terms
from tests.helpers import set_opt
from tests.test_solr_search import GOLDEN, KS, _lower_whole, check


@pytest.fixture(autouse=True)
def _device(default_api):
    yield


def synth_frame(n, fields=("title", "body", "tags"), seed=0):
    """columns of `n` seeded Zipf docs over ~50 tokens: posting lists span every tile and scores tie.  `title` knows t0..t39 only."""
    names = np.array([f"t{i}" for i in range(50)])
    cols = {}
    for j, f in enumerate(("title", "body", "tags")):
        if f not in fields:
            continue
        lens, terms = synth.zipf_batch_tokens(seed + j, n, 40 if f == "title" else 50, mean_len=3 + 4 * j)
        st = np.concatenate([[0], np.cumsum(lens)])
        cols[f] = SearchArray.index([" ".join(names[terms[st[i]:st[i + 1]]]) for i in range(n)])
    return pd.DataFrame(cols)


_frames = {}
_host = {}


@pytest.fixture(scope="module")
def frames(default_api):
    def get(n, fields=("title", "body", "tags")):
        key = (n, tuple(fields))
        if key not in _frames:
            _frames[key] = synth_frame(n, fields)
        return key, _frames[key]
    yield get
    _frames.clear()
    _host.clear()


def host(key, frame, q, params):
    """(scores, explain) of the host route, computed once per (frame, query, parameters)"""
    ck = (key, q, json.dumps(params, sort_keys=True, default=repr))
    if ck not in _host:
        _host[ck] = edismax(frame, q=q, use_device=False, **params)
    return _host[ck]


def check_batch(key, frame, queries, params, k, mask=None, fq=None, per_query=None, what=""):
    """the batch against the host route for every query, and against edismax_search alone for the queries `per_query` (None: all)"""
    hits = edismax_search_batch(frame, queries, k=k, fq=fq if fq is not None else mask, **params)
    assert isinstance(hits, list) and len(hits) == len(queries)
    wants = []
    for i, q in enumerate(queries):
        scores, explain = host(key, frame, q, params)
        check(hits[i], scores, mask, k, explain, f"{what} q{i}={q!r} k={k}")
        wants.append(scores)
        if per_query is None or i in per_query:
            one = edismax_search(frame, q, k=k, fq=fq if fq is not None else mask, **params)
            assert one.found == hits[i].found and one.explain == hits[i].explain and one.scores.dtype == hits[i].scores.dtype
            assert np.array_equal(one.rows, hits[i].rows) and np.array_equal(one.scores, hits[i].scores), f"{what} q{i} vs edismax_search"
    return hits, wants


# ---- 1. goldens: term-centric, field-centric and pf* queries in one list ---------------------------------------------------------
@pytest.fixture(scope="module")
def golden(default_api):
    g = np.load(GOLDEN, allow_pickle=False)
    frame = pd.DataFrame({"title": SearchArray.index(list(g["field_title"])),
                          "body": SearchArray.index(list(g["field_body"])),
                          "tags": SearchArray.index(list(g["field_tags"]), tokenizer=_lower_whole)})
    return g, frame, json.loads(str(g["cases"]))


def test_goldens_keep_the_properties_this_file_relies_on(golden):
    g, frame, cases = golden
    assert len(cases) == 12 and len(frame) == 300
    qs = [c["q"] for c in cases]
    kinds = set()
    for c in cases:
        for q in qs:
            n_terms, _, term_centric = parse_query_terms(frame, q, list(solr.parse_field_boosts(c["qf"])))
            kinds.add((bool(term_centric), bool(c.get("pf") or c.get("pf2") or c.get("pf3"))))
            assert n_terms <= 32
    # every route of the batch is taken: the kernel, the per-query route for one query of a list, and for a whole list (pf*)
    assert kinds >= {(True, False), (False, False), (True, True)}
    assert any(len(q.split()) >= 3 for q in qs) and any(len(q.split()) == 1 for q in qs)


@pytest.mark.parametrize("case", range(12))
def test_every_golden_query_under_every_golden_case(golden, case, on_emu):
    g, frame, cases = golden
    params = {a: v for a, v in cases[case].items() if a != "q"}
    queries = [c["q"] for c in cases]
    own = queries.index(cases[case]["q"])
    scores, explain = host(("golden",), frame, cases[case]["q"], params)
    assert np.allclose(scores, g[f"scores_{case}"], rtol=1e-6, atol=0) and explain == str(g[f"explain_{case}"])   # (the yardstick is the reference's output)
    for k in (KS[case % 2::2] if on_emu else KS):
        hits, wants = check_batch(("golden",), frame, queries, params, k, per_query={own, (own + 5) % 12} if on_emu else None,
                                  what=f"case {case}")
        if k == 10:
            assert max((w > 0).sum() for w in wants) > 10          # the selection selects


# ---- 2. tile edges ---------------------------------------------------------------------------------------------------------------
POOL = ["t1", "t0 t2", "t3 t7 t9", "t1 t4 t5 t6", "t0 t8 t2 t11 t30", "t45 t1", "t45", "zzz t3", "zzz", "t5 t5 t6", "", "t2 t2",
        "t12 t13 t14", "t20 t21", "t39 t1 zzz"]
QF2, QF3 = ["title^3", "body"], ["title^0.5", "body^2", "tags"]
SIMS = {"title": bm25_similarity(k1=0.9, b=0.4), "body": bm25_similarity(k1=1.6, b=0.3), "tags": bm25_similarity()}


def queries_of(B):
    return [POOL[i % len(POOL)] if i < len(POOL) else f"t{i % 37} t{(i * 7) % 41} t{(i * 3) % 50}" for i in range(B)]


COMBOS = [                                         # (fields, parameters, B, k)
    (2, dict(qf=QF2, tie=0.0), 65, 10),
    (3, dict(qf=QF3, tie=0.1, mm=2), 3, 10),
    (2, dict(qf=QF2, tie=1.0, mm="75%"), 1, 1),
    (3, dict(qf=QF3, tie=0.1, mm="2<75%"), 65, 1000),
    (2, dict(qf=QF2, tie=0.1, q_op="AND"), 15, 100),
    (3, dict(qf=QF3, tie=0.0, similarity=SIMS), 15, 10),
]


@pytest.mark.parametrize("combo", range(len(COMBOS)))
@pytest.mark.parametrize("n_docs", [1, 2047, 2048, 2049, 5000])
def test_tile_edges(frames, n_docs, combo, on_emu):
    n_fields, params, B, k = COMBOS[combo]
    if on_emu and B == 65 and not (n_docs == 2049 and combo == 0):
        B = 11                                      # (the emulator runs one 65-query list; the GPU all of them)
    key, frame = frames(n_docs, ("title", "body", "tags")[:n_fields])
    queries = queries_of(B)
    hits, wants = check_batch(key, frame, queries, params, k, per_query=set(range(0, B, 4)) if on_emu else None,
                              what=f"n={n_docs} {params}")
    if n_docs >= 2047 and B >= 11:
        pos = [int((w > 0).sum()) for w in wants]
        assert min(pos) == 0                                         # an unknown token, the empty query
        if k <= 100 and "q_op" not in params:
            assert max(pos) > k                                      # more matches than k somewhere
        assert any(len(np.unique(w[w > 0])) < (w > 0).sum() for w in wants)          # ties
        title = frame["title"].array
        assert title.docfreq("t45") == 0 and frame["body"].array.docfreq("t45") > 0  # unknown in one field only
        if n_docs > 2048:
            assert any(np.flatnonzero(w > 0).max() >= 2048 for w in wants if (w > 0).any())      # more than one tile holds matches


def test_all_term_centric_lists_never_take_the_per_query_route(frames, monkeypatch):
    key, frame = frames(2049, ("title", "body"))
    calls = []
    real = solr.edismax_search
    monkeypatch.setattr(solr, "edismax_search", lambda *a, **kw: calls.append(a) or real(*a, **kw))
    queries = queries_of(11)
    edismax_search_batch(frame, queries, qf=QF2, mm=2, tie=0.1)
    assert calls == []
    edismax_search_batch(frame, queries, qf=QF2, mm=2, tie=0.1, pf=["body"])         # a per-call condition: the whole list, one by one
    assert len(calls) == 11
    del calls[:]
    long_q = " ".join(f"t{i}" for i in range(33))                                    # more than 32 clauses: that query alone
    hits = edismax_search_batch(frame, [queries[1], long_q, queries[2]], qf=QF2)
    assert len(calls) == 1 and calls[0][1] == long_q
    scores, explain = host(key, frame, long_q, dict(qf=QF2))
    check(hits[1], scores, None, 10, explain, "33 terms")
    assert edismax_search_batch(frame, [], qf=QF2) == []


# ---- 3. all ties -------------------------------------------------------------------------------------------------------------------
def test_all_ties(default_api):
    n = 4500
    frame = pd.DataFrame({"title": SearchArray.index(["a b"] * n), "body": SearchArray.index(["a b"] * n)})
    queries = ["a b", "a", "b a"]
    params = dict(qf=["title^2", "body"], tie=0.1)
    drop = np.ones(n, dtype=bool)
    drop[:2048] = False
    for k in (10, 1000):
        for mask, first in ((None, 0), (drop, 2048)):
            hits, wants = check_batch(("ties",), frame, queries, params, k, mask=mask, per_query={0}, what="ties")
            for h, w in zip(hits, wants):
                assert len(np.unique(w)) == 1 and w[0] > 0
                assert np.array_equal(h.rows, np.arange(first, first + k, dtype=np.uint64)) and h.found == n - first


# ---- 4. fq forms -------------------------------------------------------------------------------------------------------------------
def test_fq_forms(frames):
    key, frame = frames(5000)
    n = len(frame)
    title, body = frame["title"].array, frame["body"].array
    queries = ["t1 t4", "t0 t8 t2", "zzz t3", "t45 t1", "t20"]
    params = dict(qf=QF3, tie=0.1, mm="2<75%")
    rng = np.random.default_rng(11)
    mask = rng.random(n) < 0.4
    rows = np.flatnonzero(mask)
    few = set(range(0, len(queries), 2))
    for k in (10, 1000):
        what = f"fq k={k}"
        _, wants = check_batch(key, frame, queries, params, k, mask=mask, per_query=few, what=what + " mask")
        check_batch(key, frame, queries, params, k, mask=mask, fq=np.concatenate([rows[::-1], rows[:3]]), per_query=few, what=what + " reversed rows with repeats")
        has_t1 = title.termfreqs("t1") > 0
        has_t2 = title.termfreqs("t2") > 0
        has_b = body.termfreqs("t7") > 0
        assert has_t1.any() and has_t2.any() and has_b.any() and not np.array_equal(has_t1, has_t2)
        f_t1, f_t2, f_mask, f_body = title.term_filter("t1"), title.term_filter("t2"), title.doc_filter(mask), body.term_filter("t7")
        both = f_t1 & ~f_t2
        mixed = (f_mask | f_t2) - f_t1
        try:
            check_batch(key, frame, queries, params, k, mask=has_b, fq=f_body, per_query=few, what=what + " another column's filter")
            check_batch(key, frame, queries, params, k, mask=has_t1 & ~has_t2, fq=both, per_query=few, what=what + " & ~")
            check_batch(key, frame, queries, params, k, mask=(mask | has_t2) & ~has_t1, fq=mixed, per_query=few, what=what + " | -")
            assert f_t1.count() == int(has_t1.sum())                          # the caller's filters are still open
        finally:
            for f in (f_t1, f_t2, f_mask, f_body, both, mixed):
                f.close()
        check_batch(key, frame, queries, params, k, mask=np.zeros(n, bool), fq=np.zeros(0, np.int64), per_query=few, what=what + " empty")
        none = np.ones(n, dtype=bool)
        for w in wants:
            none &= ~(w > 0)
        hits, _ = check_batch(key, frame, queries, params, k, mask=none, per_query=few, what=what + " every match excluded")
        assert none.any() and all(h.found == 0 and np.all(h.rows == NO_DOC) and np.all(h.scores == 0) for h in hits)
        band = np.zeros(n, dtype=bool)
        band[2048:4096] = True                                                # the first and the last tile hold nothing eligible
        hits, _ = check_batch(key, frame, queries, params, k, mask=band, per_query=few, what=what + " range")
        assert any(h.found > 0 for h in hits)


# ---- 6. slices through the Python surface ----------------------------------------------------------------------------------------
def test_sliced_call_equals_unsliced(frames, on_emu):
    key, frame = frames(5000, ("title", "body"))
    queries = queries_of(65 if not on_emu else 33)
    params = dict(qf=QF2, tie=0.1, mm=2)
    whole = edismax_search_batch(frame, queries, k=1000, **params)
    set_opt("fields_cand_mb", 1)                    # 3 tiles x 1000 candidates x 12 bytes per query: 29 queries in flight at most
    sliced = edismax_search_batch(frame, queries, k=1000, **params)
    for a, b in zip(whole, sliced):
        assert a.found == b.found and a.explain == b.explain and np.array_equal(a.rows, b.rows) and np.array_equal(a.scores, b.scores)


# ---- 7. threads --------------------------------------------------------------------------------------------------------------------
def test_two_threads_equal_serial(frames):
    key, frame = frames(2049, ("title", "body"))
    queries = queries_of(11)
    params = dict(qf=QF2, tie=0.3, mm=2, k=20)
    serial = edismax_search_batch(frame, queries, **params)
    for i, q in enumerate(queries):
        scores, explain = host(key, frame, q, dict(qf=QF2, tie=0.3, mm=2))
        check(serial[i], scores, None, 20, explain, f"serial {q!r}")
    got, errors = {}, []

    def work(name):
        try:
            got[name] = [edismax_search_batch(frame, queries, **params) for _ in range(2)]
        except Exception as e:                      # (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for runs in got.values():
        for hits in runs:
            for a, b in zip(serial, hits):
                assert a.found == b.found and a.explain == b.explain and np.array_equal(a.rows, b.rows) and np.array_equal(a.scores, b.scores)


# ---- 8. errors and fallbacks -------------------------------------------------------------------------------------------------------
def test_errors_match_edismax_search(frames):
    key, frame = frames(2049, ("title", "body"))
    n = len(frame)
    queries = ["t1 t2", "t3"]
    for route in (None, False):
        for bad_k in (0, 1025):
            with pytest.raises(ValueError, match="k must be in 1 .. 1024"):
                edismax_search_batch(frame, queries, qf=QF2, k=bad_k, use_device=route)
        for bad_fq, msg in ((np.ones(n + 1, bool), "one entry per row"), (np.asarray([0, n]), "row ids must lie"),
                            (np.asarray([-1, 2]), "row ids must lie")):
            with pytest.raises(ValueError, match=msg) as batch_err:
                edismax_search_batch(frame, queries, qf=QF2, fq=bad_fq, use_device=route)
            with pytest.raises(ValueError, match=msg) as one_err:
                edismax_search(frame, queries[0], qf=QF2, fq=bad_fq, use_device=route)
            assert str(batch_err.value) == str(one_err.value)
    short = SearchArray.index(["a b", "b c"])
    f = short.doc_filter(np.asarray([True, False]))
    try:
        with pytest.raises(ValueError, match="fq covers 2 documents"):
            edismax_search_batch(frame, queries, qf=QF2, fq=f)
    finally:
        f.close()
    with pytest.raises(ValueError, match="not in dataframe"):
        edismax_search_batch(frame, queries, qf=["nope"])


def test_fallbacks_are_still_equal(frames):
    # nine fields: more than a fields batch spans
    names = np.array([f"t{i}" for i in range(20)])
    cols = {}
    for j in range(9):
        lens, terms = synth.zipf_batch_tokens(50 + j, 120, 20, mean_len=4)
        st = np.concatenate([[0], np.cumsum(lens)])
        cols[f"f{j}"] = SearchArray.index([" ".join(names[terms[st[i]:st[i + 1]]]) for i in range(120)])
    wide = pd.DataFrame(cols)
    check_batch(("wide",), wide, ["t1 t2", "t3", "zzz"], dict(qf=[f"f{j}^{1 + j}" for j in range(9)], tie=0.2), 10, what="nine fields")
    # the host route, a negative boost (host route by edismax's own rule) and a custom similarity
    key, frame = frames(2049, ("title", "body"))
    mask = np.arange(len(frame)) % 3 == 0
    for params in (dict(qf=QF2, use_device=False), dict(qf=["title^-2", "body"])):
        hits = edismax_search_batch(frame, ["t1 t2", "t3"], k=10, fq=mask, **params)
        for q, h in zip(["t1 t2", "t3"], hits):
            scores, explain = edismax(frame, q=q, **params)
            check(h, scores, mask, 10, explain, f"{params}")
