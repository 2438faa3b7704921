"""Solr-style query helpers on top of ``SearchArray`` columns: ``edismax`` and the ``mm`` grammar.

Same public names, arguments and results as the reference's ``searcharray/solr.py`` (v0.0.73) --
``parse_min_should_match`` (solr.py:10-60), ``parse_field_boosts`` (:63-75), ``edismax`` (:239-355) --
so code written against the reference runs unchanged; the scoring calls underneath are
``SearchArray.score`` on the GPU.  The combination rules, including two behaviours that look
accidental but are observable, are the reference's:

* term-centric when every query field tokenises the query into the same number of terms
  (solr.py:87-109, 112-144), field-centric otherwise (:147-176);
* phrase boosts (pf / pf2 / pf3) are computed on the docs the main query matched and added there
  (:320-353); in the pf2 phase the LAST bigram of every field is added twice (:210-218).

With stock BM25 similarities on whole (unsliced) arrays the combination itself runs on the GPU
(``_DeviceCombiner``: Part 4 of the C ABI, csrc/sa_vec.hip): every per-field, per-term score is computed
straight into a device vector and only the final result crosses PCIe.  The arithmetic follows numpy's
operation for operation, so both routes return identical arrays (tests/test_solr.py runs each scenario
through both).  Anything else -- custom similarity callables, slices -- takes the host route.

``edismax_search`` (no counterpart in the reference, whose callers rank the dense result with ``np.argpartition``) returns the
top ``k`` rows of the same scores, optionally inside a document filter (Solr's ``fq``): on the device route the combined vector
is selected in HBM (``sa_vec_topk``, csrc/sa_vec_topk.hip) and never crosses PCIe.  ``edismax_facets`` counts the same vector
instead of ranking it -- Solr's ``facet.field`` for one query (``sa_vec_facet_counts``, csrc/sa_facet.hip).
"""
from __future__ import annotations

import ctypes
import re
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import pandas as pd

from .device_index import NO_DOC, DocFilter, FacetColumn, FacetCounts
from .postings import SearchArray
from .similarity import Similarity, default_bm25

_INT_ERR = "Invalid 'mm' spec. Expecting an integer."
_F32P = ctypes.POINTER(ctypes.c_float)


def _mm_int(text: str) -> int:
    try:
        return int(text)
    except ValueError:
        raise ValueError(_INT_ERR)


def _mm_simple(num_clauses: int, result: int, spec: str) -> int:
    """``N``, ``-N``, ``P%`` or ``-P%`` applied to ``result`` clauses (reference solr.py:47-60)."""
    if "%" in spec:
        share = (result * _mm_int(spec[:-1])) * (1 / 100)       # '%' is assumed to be the last character
        result = result + int(share) if share < 0 else int(share)
    else:
        n = _mm_int(spec)
        result = result + n if n < 0 else n
    return min(num_clauses, max(result, 0))


def parse_min_should_match(num_clauses: int, spec: str) -> int:
    """Solr's ``mm`` ("minimum should match") grammar: how many of ``num_clauses`` optional clauses a
    document must match.  ``"3"``, ``"-2"``, ``"75%"``, ``"-25%"`` and conditional lists such as
    ``"2<-25% 9<-3"`` (the rule after the largest bound below ``num_clauses`` applies)."""
    spec = spec.strip()
    if "<" not in spec:
        return _mm_simple(num_clauses, num_clauses, spec)
    required = num_clauses
    for rule in re.sub(r"\s*<\s*", "<", spec).split():
        bound, sep, then = rule.partition("<")
        if not sep:
            raise ValueError("Invalid 'mm' spec: '" + rule + "'. Expecting values before and after '<'")
        if num_clauses <= _mm_int(bound):
            return required
        required = parse_min_should_match(num_clauses, then)
    return required


OCCUR_SHOULD, OCCUR_MUST, OCCUR_MUST_NOT = 0, 1, 2
_OCCUR_SYMBOLS = {"": OCCUR_SHOULD, "should": OCCUR_SHOULD, "+": OCCUR_MUST, "must": OCCUR_MUST, "-": OCCUR_MUST_NOT,
                  "must_not": OCCUR_MUST_NOT}


def occur_class(symbol) -> int:
    """one occur symbol of ``SearchArray.search(occur=...)`` -> 0 (should), 1 (must), 2 (must_not): ``""`` / ``"should"`` / 0,
    ``"+"`` / ``"must"`` / 1, ``"-"`` / ``"must_not"`` / 2"""
    if isinstance(symbol, str):
        if symbol in _OCCUR_SYMBOLS:
            return _OCCUR_SYMBOLS[symbol]
    elif not isinstance(symbol, bool) and isinstance(symbol, (int, np.integer)) and 0 <= int(symbol) <= 2:
        return int(symbol)
    raise ValueError(f"occur symbols are '+' / 'must' / 1, '-' / 'must_not' / 2 and '' / 'should' / 0, got {symbol!r}")


def split_occur(query_or_tokens, tokenizer) -> Tuple[List[str], List[int]]:
    """The ``+tok`` / ``-tok`` prefixes of a Lucene / Solr query, read once: ``(tokens, classes)`` with one class (0 should, 1 must,
    2 must_not) per token, ready for ``SearchArray.search(tokens_per_query, occur=classes_per_query)``.
    A string is split on whitespace into clauses; one leading ``+`` / ``-`` of a clause is stripped and the rest is run through
    ``tokenizer`` -- every token a clause yields inherits the clause's class.  In a token list one leading ``+`` / ``-`` of each token
    is stripped (``tokenizer`` is not applied).  A clause or token that is nothing but the sign is left as it is."""
    def sign(text):
        if len(text) > 1 and text[0] in "+-":
            return text[1:], OCCUR_MUST if text[0] == "+" else OCCUR_MUST_NOT
        return text, OCCUR_SHOULD

    tokens: List[str] = []
    classes: List[int] = []
    if isinstance(query_or_tokens, str):
        for clause in query_or_tokens.split():
            rest, cls = sign(clause)
            for tok in tokenizer(rest):
                tokens.append(tok)
                classes.append(cls)
    else:
        for tok in query_or_tokens:
            if not isinstance(tok, str):
                raise TypeError("Expected a string")
            rest, cls = sign(tok)
            tokens.append(rest)
            classes.append(cls)
    return tokens, classes


def parse_field_boosts(field_lists: Optional[Sequence[str]]) -> Dict[str, Optional[float]]:
    """``["title^10", "body"]`` -> ``{"title": 10.0, "body": None}`` (qf, pf, pf2, pf3)."""
    boosts: Dict[str, Optional[float]] = {}
    for spec in field_lists or []:
        pieces = spec.split("^")
        boosts[pieces[0]] = float(pieces[1]) if len(pieces) > 1 else None
    return boosts


def get_field(frame: pd.DataFrame, field: str) -> SearchArray:
    if field not in frame.columns:
        raise ValueError(f"Field {field} not in dataframe")
    column = frame[field].array
    if not isinstance(column, SearchArray):
        raise ValueError(f"Field {field} is not a searcharray field")
    return column


def _weight(boost: Optional[float]) -> float:
    return 1 if boost is None else boost


def _boost_text(boost: Optional[float]) -> str:
    return "1" if boost is None else f"{boost}"


@dataclass
class _Field:
    name: str
    boost: Optional[float]
    array: SearchArray
    terms: List[str]
    similarity: Similarity


def parse_query_terms(frame: pd.DataFrame, query: str, query_fields: Sequence[str]):
    """Tokenise ``query`` with every field's own tokenizer.  Term-centric scoring needs the same
    number of terms from every field."""
    per_field = {f: list(get_field(frame, f).tokenizer(query)) for f in query_fields}
    counts = [len(t) for t in per_field.values()]
    n_terms = next((c for c in counts if c), 0)
    # the reference compares every later field with the first non-zero count (solr.py:103-107)
    term_centric = True
    seen = 0
    for c in counts:
        if seen == 0:
            seen = c
        elif c != seen:
            term_centric = False
    return n_terms, per_field, term_centric


def _dismax(per_field_scores: np.ndarray, tie: float) -> np.ndarray:
    """disjunction-max over axis 0 with a tie breaker: max + tie * (sum - max)"""
    best = per_field_scores.max(axis=0)
    return best + (per_field_scores.sum(axis=0) - best) * tie


def _term_centric(fields: List[_Field], n_docs: int, n_terms: int, mm: str, tie: float) -> Tuple[np.ndarray, str]:
    clause_scores = np.zeros((n_terms, n_docs), dtype=np.float64)
    clauses = []
    for posn in range(n_terms):
        # float64 accumulators like the reference's np.zeros(len(frame)) (solr.py:124-125)
        stack = np.zeros((len(fields) + 1, n_docs), dtype=np.float64)
        parts = []
        for i, f in enumerate(fields):
            term = f.terms[posn]
            stack[i] = f.array.score(term, similarity=f.similarity) * _weight(f.boost)
            parts.append(f"{f.name}:{term}^{_boost_text(f.boost)}")
        total = np.zeros(n_docs)
        for i in range(len(fields)):
            total += stack[i]                                   # same left-to-right order as the reference
        best = stack.max(axis=0)
        clause_scores[posn] = best + (total - best) * tie
        clauses.append("(" + " | ".join(parts) + ")")
    need = parse_min_should_match(n_terms, spec=mm)
    enough = (clause_scores > 0).sum(axis=0) >= need
    scores = np.sum(list(clause_scores), axis=0) if n_terms else np.zeros(n_docs)
    scores[~enough] = 0
    return scores, "(" + " ".join(clauses) + f")~{need}"


def _field_centric(fields: List[_Field], n_docs: int, mm: str, tie: float) -> Tuple[np.ndarray, str]:
    rows = []
    texts = []
    for f in fields:
        per_term = np.array([f.array.score(t, similarity=f.similarity) for t in f.terms])
        need = min(parse_min_should_match(len(f.terms), spec=mm), len(f.terms))
        enough = np.sum(per_term > 0, axis=0) >= need
        summed = np.sum(per_term, axis=0)
        summed[~enough] = 0
        rows.append(summed * _weight(f.boost))
        clause = " ".join(f"{f.name}:{t}" for t in f.terms)
        texts.append(f"(({clause})~{need})^{_boost_text(f.boost)}")
    return _dismax(np.asarray(rows), tie), " | ".join(texts)


def _ngrams(terms: List[str], n: int):
    return [terms[i:i + n] for i in range(len(terms) - n + 1)]


def _phrase_phase(matched: Dict[str, SearchArray], per_field: Dict[str, List[str]], boosts: Dict[str, Optional[float]],
                  similarity: Dict[str, Similarity], n: Optional[int]):
    """Sum of the boosted phrase scores over the matched docs.  n=None: the whole query as one phrase
    (pf, needs >= 2 terms); n=2 / n=3: every bigram / trigram (pf2 / pf3)."""
    pieces: List[np.ndarray] = []
    text = ""
    for field, boost in boosts.items():
        terms = per_field[field]
        if len(terms) < (2 if n is None else n):
            continue
        grams = [terms] if n is None else _ngrams(terms, n)
        last = None
        for gram in grams:
            last = matched[field].score(list(gram), similarity=similarity[field]) * _weight(boost)
            text += f" ({field}:\"{' '.join(gram)}\")^{_boost_text(boost)}"
            pieces.append(last)
        if n == 2 and last is not None:
            pieces.append(last)            # reference solr.py:217: the field's last bigram counts twice
    return (np.sum(pieces, axis=0) if pieces else None), text


class _DeviceCombiner:
    """The edismax combination on device vectors; mirrors _term_centric / _field_centric / _phrase_phase."""

    def __init__(self, fields: List[_Field], n_docs: int):
        from .device_index import DeviceVec
        self.fields = fields
        self.n = n_docs
        self.devs = {f.name: f.array._core.device() for f in fields}
        self.api = next(iter(self.devs.values())).api
        self._Vec = DeviceVec
        self._vecs = []

    @staticmethod
    def usable(fields: List[_Field], n_docs: int) -> bool:
        if n_docs == 0 or not fields:
            return False
        for f in fields:
            sim = f.similarity
            if getattr(sim, "kind", None) != "bm25" or sim.k1 == 0 or sim.b == 1:
                return False
            # a negative boost makes the main-query scores mixed-sign; the reference then slices with
            # `scores > 0` but adds at `np.where(scores)` and raises a broadcast ValueError
            # (solr.py:320-353): only the host route reproduces that
            if f.boost is not None and f.boost < 0:
                return False
            if f.array._rows is not None or len(f.array) != n_docs or len(f.array._core.doc_lens) == 0:
                return False
        return True

    def vec(self, f64: bool):
        v = self._Vec(self.api, self.n, f64)
        self._vecs.append(v)
        return v

    def close(self):
        for v in self._vecs:
            v.close()
        self._vecs = []

    # one term or phrase of one field -> float32 vector (times boost), idf from the given docfreqs
    def score_into(self, out, f: _Field, tokens: List[str], boost, dfs=None):
        from .device_index import NO_TERM, compute_idf, p_u32
        arr, dev = f.array, self.devs[f.name]
        ids = [arr._term_id(t) for t in tokens]
        tarr = np.asarray([i if i >= 0 else NO_TERM for i in ids], dtype=np.uint32)
        if dfs is None:
            dfs = np.asarray([arr.docfreq(t) for t in tokens])
        idf = np.float32(compute_idf(arr.corpus_size, np.asarray(dfs)))
        k1, b = np.float32(f.similarity.k1), np.float32(f.similarity.b)
        if len(tokens) == 1:
            dev.into_vec(out, boost, "sa_index_bm25_dense", p_u32(tarr), np.asarray([idf], np.float32).ctypes.data_as(_F32P), 1, k1, b)
        else:
            dev.into_vec(out, boost, "sa_index_bm25_phrase_dense_posn", p_u32(tarr), len(tarr), 0, -1, -1, idf, k1, b)

    def term_centric(self, n_terms: int, need: int, tie: float):
        call = self.api.call
        total, cnt = self.vec(True), self.vec(False)
        acc, best, s = self.vec(True), self.vec(True), self.vec(False)
        for posn in range(n_terms):
            acc.zero()
            best.zero()
            for f in self.fields:
                self.score_into(s, f, [f.terms[posn]], f.boost)
                call("sa_vec_dismax_acc", acc._h, best._h, s._h)
            call("sa_vec_clause", acc._h, best._h, float(tie), total._h, cnt._h)
        call("sa_vec_mask_min_count", total._h, cnt._h, int(need))
        return total

    def field_centric(self, mm: str, tie: float):
        call = self.api.call
        fsum, fmax, out = self.vec(False), self.vec(False), self.vec(False)
        summed, cnt, s = self.vec(False), self.vec(False), self.vec(False)
        for k, f in enumerate(self.fields):
            summed.zero()
            cnt.zero()
            for t in f.terms:
                self.score_into(s, f, [t], None)
                call("sa_vec_sum_count32", summed._h, cnt._h, s._h)
            need = min(parse_min_should_match(len(f.terms), spec=mm), len(f.terms))
            call("sa_vec_field_row", summed._h, cnt._h, int(need), np.float32(_weight(f.boost)), 0 if f.boost is None else 1,
                 1 if k == 0 else 0, fsum._h, fmax._h)
        call("sa_vec_field_finish", fsum._h, fmax._h, np.float32(tie), out._h)
        return out

    def phrase_phase(self, scores, mask0, per_field, boosts, n):
        """scores[matched] += sum of the boosted phrase scores computed with the matched docs' docfreqs"""
        from .device_index import NO_TERM
        call = self.api.call
        by_name = {f.name: f for f in self.fields}
        extra, piece, tf = self.vec(False), self.vec(False), self.vec(False)
        n_pieces = 0
        for field, boost in boosts.items():
            terms = per_field[field]
            if len(terms) < (2 if n is None else n):
                continue
            f = by_name[field]                       # KeyError for a phrase field outside qf, as in the reference
            dev = self.devs[field]
            grams = [terms] if n is None else _ngrams(terms, n)
            if n == 2:
                grams = grams + [grams[-1]]          # reference solr.py:217: the field's last bigram counts twice
            for gram in grams:
                dfs = []
                for tok in gram:                     # docfreq among the matched docs (slices are subset-local)
                    tid = f.array._term_id(tok)
                    c = ctypes.c_uint64(0)
                    if tid >= 0:
                        dev.into_vec(tf, None, "sa_index_termfreqs_dense_posn", tid, -1, -1)
                        call("sa_vec_count_where", tf._h, mask0._h, ctypes.byref(c))
                    dfs.append(c.value)
                self.score_into(piece, f, list(gram), boost, dfs=dfs)
                call("sa_vec_add32", extra._h, piece._h, 1 if n_pieces == 0 else 0)
                n_pieces += 1
        if n_pieces:
            call("sa_vec_add_where", scores._h, extra._h, scores._h)


class _Plan(NamedTuple):
    """an edismax call with its arguments resolved: what both routes and both entry points start from"""
    fields: List[_Field]
    per_field: Dict[str, List[str]]
    similarity: Dict[str, Similarity]
    n_terms: int
    term_centric: bool
    mm: str
    phases: tuple


def _plan(frame, q, qf, mm, pf, pf2, pf3, q_op, similarity) -> _Plan:
    def as_list(x):
        return x if isinstance(x, list) else [x]

    query_boosts = parse_field_boosts(as_list(qf))
    phrase_boosts = parse_field_boosts(as_list(pf)) if pf else {}
    bigram_boosts = parse_field_boosts(pf2) if pf2 else {}
    trigram_boosts = parse_field_boosts(pf3) if pf3 else {}
    mm = "1" if mm is None else (f"{mm}" if isinstance(mm, int) else mm)
    if q_op == "AND":
        mm = "100%"
    if not isinstance(similarity, dict):
        similarity = {field: similarity for field in query_boosts}
    for field in query_boosts:
        similarity.setdefault(field, default_bm25)

    n_terms, per_field, term_centric = parse_query_terms(frame, q, list(query_boosts))
    fields = [_Field(name, boost, get_field(frame, name), per_field[name], similarity[name])
              for name, boost in query_boosts.items()]
    phases = ((phrase_boosts, None), (bigram_boosts, 2), (trigram_boosts, 3))
    return _Plan(fields, per_field, similarity, n_terms, term_centric, mm, phases)


def _device_scores(comb: _DeviceCombiner, plan: _Plan, tie: float):
    """the combined scores as a device vector of ``comb`` (closed with it) and the explain string, which is the host route's"""
    if plan.term_centric:
        need = parse_min_should_match(plan.n_terms, spec=plan.mm)
        scores_v = comb.term_centric(plan.n_terms, need, tie)
    else:
        scores_v = comb.field_centric(plan.mm, tie)
    explain = _explain_main(plan.fields, plan.n_terms, plan.mm, plan.term_centric)
    mask0 = comb.vec(scores_v.f64)
    mask0.copy_from(scores_v)
    for boosts, n in plan.phases:
        comb.phrase_phase(scores_v, mask0, plan.per_field, boosts, n)
        explain += _explain_phase(plan.per_field, boosts, n)
    return scores_v, explain


def _host_scores(frame: pd.DataFrame, plan: _Plan, tie: float) -> Tuple[np.ndarray, str]:
    fields = plan.fields
    if plan.term_centric:
        scores, explain = _term_centric(fields, len(frame), plan.n_terms, plan.mm, tie)
    else:
        scores, explain = _field_centric(fields, len(frame), plan.mm, tie)

    # phrase boosts only look at (and only add to) the docs the main query matched
    hit = scores > 0
    matched = {f.name: f.array[hit] for f in fields}
    for boosts, n in plan.phases:
        extra, text = _phrase_phase(matched, plan.per_field, boosts, plan.similarity, n)
        explain += text
        if extra is not None:
            scores[np.where(scores)[0]] += extra
    return scores, explain


def edismax(frame: pd.DataFrame,
            q: str,
            qf: List[str],
            mm: Optional[Union[str, int]] = None,
            pf: Optional[List[str]] = None,
            pf2: Optional[List[str]] = None,
            pf3: Optional[List[str]] = None,
            ps2: int = 0,
            ps3: int = 0,
            ps: int = 0,
            tie: float = 0.0,
            q_op: str = "OR",
            similarity: Union[Similarity, Dict[str, Similarity]] = default_bm25,
            use_device: Optional[bool] = None) -> Tuple[np.ndarray, str]:
    """Solr's extended-dismax over a dataframe whose ``qf`` columns are ``SearchArray`` s.

    q: query string; qf: fields with optional ``^boost``; mm: minimum-should-match spec (default
    ``"1"``; ``q_op="AND"`` forces ``"100%"``); pf / pf2 / pf3: fields boosted when the whole query /
    its bigrams / its trigrams match as a phrase; tie: dismax tie breaker; similarity: one callable or
    one per field.  ps / ps2 / ps3 are accepted for signature parity and, as in the reference, unused.
    use_device: None picks the GPU combination whenever it applies (stock BM25, unsliced arrays); False
    forces the host route.  Returns ``(scores[len(frame)], explain string)`` -- float64 term-centric,
    float32 field-centric, as the reference.  :func:`edismax_search` ranks the same scores on the device
    and returns the top ``k`` instead of the dense vector."""
    plan = _plan(frame, q, qf, mm, pf, pf2, pf3, q_op, similarity)
    if use_device is None:
        use_device = _DeviceCombiner.usable(plan.fields, len(frame))
    if use_device:
        # everything stays in HBM until the final vector
        comb = _DeviceCombiner(plan.fields, len(frame))
        try:
            scores_v, explain = _device_scores(comb, plan, tie)
            return scores_v.fetch(), explain
        finally:
            comb.close()
    return _host_scores(frame, plan, tie)


class SearchHits(NamedTuple):
    """what :func:`edismax_search` returns: the ``k`` best rows of the frame, best first"""
    scores: np.ndarray       # float64 (term-centric) or float32 (field-centric), as edismax's vector; 0 past the hits
    rows: np.ndarray         # uint64 row positions in the frame; 2**64 - 1 (NO_DOC) past the hits
    found: int               # rows with a score > 0 inside fq, whatever k is (Solr's numFound)
    explain: str


def _fq_mask(frame: pd.DataFrame, fq) -> Optional[np.ndarray]:
    """``fq`` as a boolean mask of the frame's rows (None: no filter); checks it as ``SearchArray.search(filter=)`` does"""
    if fq is None:
        return None
    if isinstance(fq, DocFilter):
        if fq.index.n_docs != len(frame):
            raise ValueError(f"fq covers {fq.index.n_docs} documents, the frame has {len(frame)} rows")
        return fq.to_mask()
    a = np.asarray(fq)
    n = len(frame)
    if a.dtype == bool:
        if a.shape != (n,):
            raise ValueError(f"a boolean fq needs one entry per row ({n}), got shape {a.shape}")
        return a
    if a.size == 0:
        return np.zeros(n, dtype=bool)
    if a.dtype.kind not in "iu" or a.ndim != 1:
        raise ValueError("fq: a boolean mask of len(frame), a 1-d integer array of row ids, or a DocFilter")
    if int(a.min()) < 0 or int(a.max()) >= n:
        raise ValueError(f"fq row ids must lie in [0, {n})")
    mask = np.zeros(n, dtype=bool)
    mask[a] = True
    return mask


def _host_topk(scores: np.ndarray, mask: Optional[np.ndarray], k: int):
    """numpy selection in the device's order: positives only, value descending, then row ascending"""
    keep = scores > 0
    if mask is not None:
        keep &= mask
    idx = np.flatnonzero(keep)
    order = idx[np.lexsort((idx, -scores[idx]))[:k]]
    out_s = np.zeros(k, dtype=scores.dtype)
    out_r = np.full(k, NO_DOC, dtype=np.uint64)
    out_s[:len(order)] = scores[order]
    out_r[:len(order)] = order
    return out_s, out_r, int(len(idx))


def edismax_search(frame: pd.DataFrame,
                   q: str,
                   qf: List[str],
                   k: int = 10,
                   fq=None,
                   mm: Optional[Union[str, int]] = None,
                   pf: Optional[List[str]] = None,
                   pf2: Optional[List[str]] = None,
                   pf3: Optional[List[str]] = None,
                   ps2: int = 0,
                   ps3: int = 0,
                   ps: int = 0,
                   tie: float = 0.0,
                   q_op: str = "OR",
                   similarity: Union[Similarity, Dict[str, Similarity]] = default_bm25,
                   use_device: Optional[bool] = None) -> SearchHits:
    """:func:`edismax` ranked: the ``k`` best rows instead of one score per row.  On the device route (whenever ``edismax``
    combines on the GPU) the score vector is built exactly as ``edismax`` builds it and then selected in HBM
    (``DeviceVec.topk``): k scores and k row ids cross PCIe, not ``len(frame)`` floats.  Same keyword arguments as ``edismax``.

    Returns ``SearchHits(scores, rows, found, explain)``: only scores > 0 rank, ordered by score descending, then row
    ascending; ``scores`` has the dtype of ``edismax``'s vector; slots past the hits hold score 0 and row ``2**64 - 1``;
    ``found`` counts the rows that could rank whatever ``k`` is.  1 <= k <= 1024.

    ``fq``: rank inside a subset of the rows, as a Solr ``fq`` does -- a boolean mask of ``len(frame)``, an integer array of
    row ids, or a reusable ``DocFilter`` built from any ``SearchArray`` column of the frame (``arr.doc_filter(...)``,
    ``arr.term_filter("tok")`` and their ``& | - ~`` combinations).  The result is the top-``k`` of the unfiltered ``edismax``
    scores with the excluded rows' scores set to 0: idf, average doc length and corpus size stay those of the WHOLE columns,
    and ``mm`` and the phrase-boost phases (which use the docs the main query matched) do not see the filter.  This is not the
    reference's slice semantics (``frame[rows]`` recomputes docfreq inside the slice).

    A list of queries per call: :func:`edismax_search_batch`.  Not covered: sharded frames (``devices=``), and filters for the queue."""
    k = int(k)
    if not 1 <= k <= 1024:
        raise ValueError("k must be in 1 .. 1024")
    plan = _plan(frame, q, qf, mm, pf, pf2, pf3, q_op, similarity)
    if use_device is None:
        use_device = _DeviceCombiner.usable(plan.fields, len(frame))
    if not use_device:
        mask = _fq_mask(frame, fq)
        scores, explain = _host_scores(frame, plan, tie)
        return SearchHits(*_host_topk(scores, mask, k), explain)
    own = None                                                   # a filter made here from a mask or row ids
    if fq is None or isinstance(fq, DocFilter):
        filt = fq
        if filt is not None and filt.index.n_docs != len(frame):
            raise ValueError(f"fq covers {filt.index.n_docs} documents, the frame has {len(frame)} rows")
    else:
        mask = _fq_mask(frame, fq)         # (checked before anything is launched)
        filt = own = plan.fields[0].array._core.device().doc_filter(mask=mask)
    comb = _DeviceCombiner(plan.fields, len(frame))
    try:
        scores_v, explain = _device_scores(comb, plan, tie)
        return SearchHits(*scores_v.topk(k, filter=filt), explain)
    finally:
        comb.close()
        if own is not None:
            own.close()


def edismax_facets(frame: pd.DataFrame,
                   q: str,
                   qf: List[str],
                   by,
                   fq=None,
                   mm: Optional[Union[str, int]] = None,
                   pf: Optional[List[str]] = None,
                   pf2: Optional[List[str]] = None,
                   pf3: Optional[List[str]] = None,
                   tie: float = 0.0,
                   q_op: str = "OR",
                   similarity: Union[Similarity, Dict[str, Similarity]] = default_bm25,
                   use_device: Optional[bool] = None) -> FacetCounts:
    """Solr's ``facet.field`` for one :func:`edismax` query: how the rows it matches (score > 0, inside ``fq``) spread over a
    categorical column.  ``by``: a ``FacetColumn`` built from any ``SearchArray`` column of the frame
    (``arr.facet_column(frame.brand)``), or anything ``facet_column`` takes.  Returns ``FacetCounts(found, missing, counts
    int64[V], categories)``; ``found`` equals ``edismax_search(...).found`` for the same arguments.  On the device route the
    combined vector is counted in HBM (``sa_vec_facet_counts``): two counters and V counts cross PCIe.  Where the combination
    takes the host route (custom similarities, slices) the same numbers come from ``np.bincount`` over the host scores."""
    plan = _plan(frame, q, qf, mm, pf, pf2, pf3, q_op, similarity)
    if use_device is None:
        use_device = _DeviceCombiner.usable(plan.fields, len(frame))
    n = len(frame)
    if not use_device:
        if isinstance(by, FacetColumn):
            raise ValueError("the host route counts over host codes: pass the column's values, not a FacetColumn")
        if isinstance(by, pd.Series) and isinstance(by.dtype, pd.CategoricalDtype):
            by = by.array
        categories = by.categories if isinstance(by, pd.Categorical) else None
        codes = np.asarray(by.codes if isinstance(by, pd.Categorical) else by)
        if codes.shape != (n,) or (codes.size and codes.dtype.kind not in "iu"):
            raise ValueError(f"a facet column needs one integer code per row ({n})")
        n_values = max(1, len(categories)) if categories is not None else (max(1, int(codes.max()) + 1) if codes.size else 1)
        if codes.size and int(codes.min()) < -1:
            raise ValueError("facet codes must be -1 (no value) or >= 0")
        mask = _fq_mask(frame, fq)
        scores, _ = _host_scores(frame, plan, tie)
        keep = scores > 0
        if mask is not None:
            keep &= mask
        counts = np.bincount(codes[keep & (codes >= 0)], minlength=n_values).astype(np.int64)
        return FacetCounts(int(keep.sum()), int((keep & (codes < 0)).sum()), counts, categories)
    own = own_col = None
    if fq is None or isinstance(fq, DocFilter):
        filt = fq
        if filt is not None and filt.index.n_docs != n:
            raise ValueError(f"fq covers {filt.index.n_docs} documents, the frame has {n} rows")
    else:
        mask = _fq_mask(frame, fq)         # (checked before anything is launched)
        filt = own = plan.fields[0].array._core.device().doc_filter(mask=mask)
    comb = None
    try:
        if not isinstance(by, FacetColumn):
            by = own_col = plan.fields[0].array.facet_column(by)
        elif by.index.n_docs != n:
            raise ValueError(f"the facet column covers {by.index.n_docs} documents, the frame has {n} rows")
        comb = _DeviceCombiner(plan.fields, n)
        scores_v, _ = _device_scores(comb, plan, tie)
        found, missing, counts = scores_v.facet_counts(by, filter=filt)
        return FacetCounts(found, missing, counts, by.categories)
    finally:
        if comb is not None:
            comb.close()
        if own is not None:
            own.close()
        if own_col is not None:
            own_col.close()


_BATCH_MAX_FIELDS = 8           # a fields batch spans at most this many columns (sa_fields_batch_create)
_BATCH_MAX_TERMS = 32           # ... and a query at most this many clauses (SA_MAX_QTERMS)


def _fields_batch_inputs(plans: List[_Plan], picked: Sequence[int]):
    """what a fields batch takes for the queries ``plans[i], i in picked`` (term-centric, 1 .. 32 terms, same fields): term ids
    int64[B][T][F] (-1: the field lacks the token, or a padding clause), weights float32[B][T][F], need uint32[B]"""
    from .device_index import compute_idf
    F = len(plans[picked[0]].fields)
    T = max(plans[i].n_terms for i in picked)
    terms = np.full((len(picked), T, F), -1, dtype=np.int64)
    weights = np.zeros((len(picked), T, F), dtype=np.float32)
    need = np.zeros(len(picked), dtype=np.uint32)
    seen: Dict[Tuple[int, str], Tuple[int, np.float32]] = {}
    for row, i in enumerate(picked):
        plan = plans[i]
        need[row] = parse_min_should_match(plan.n_terms, spec=plan.mm)
        for j, f in enumerate(plan.fields):
            for posn, tok in enumerate(f.terms):
                hit = seen.get((j, tok))
                if hit is None:
                    # (what _DeviceCombiner.score_into passes: the id, and the float32 idf of the token's docfreq)
                    idf = np.float32(compute_idf(f.array.corpus_size, np.asarray([f.array.docfreq(tok)])))
                    hit = seen[(j, tok)] = (f.array._term_id(tok), idf)
                terms[row, posn, j], weights[row, posn, j] = hit
    return terms, weights, need


def _fields_batch_open(fields: List[_Field]):
    """a ``FieldsBatch`` (Part 4b of the C ABI, csrc/sa_fields.hip) over the fields' device indexes, with their BM25 parameters and boosts"""
    from .device_index import FieldsBatch
    return FieldsBatch([f.array._core.device() for f in fields], [np.float32(f.similarity.k1) for f in fields],
                       [np.float32(f.similarity.b) for f in fields], [f.boost for f in fields])


def _fields_batch_hits(plans: List[_Plan], picked: List[int], k: int, tie: float, filt) -> Optional[List[SearchHits]]:
    """the queries ``plans[i], i in picked`` ranked by ONE fields batch; None when the library cannot build one for these fields
    (no impact stream): the caller then answers them one by one"""
    from ._lib import SearchArrayHipError
    terms, weights, need = _fields_batch_inputs(plans, picked)
    try:
        fb = _fields_batch_open(plans[picked[0]].fields)
    except SearchArrayHipError:
        return None
    try:
        if filt is not None:
            fb.set_filter(filt)
        fb.set_queries(terms, weights, need, k=k, tie=tie)
        fb.run(sync=False)
        scores, rows, found = fb.fetch()
    finally:
        fb.close()
    return [SearchHits(scores[row].copy(), rows[row].copy(), int(found[row]),
                       _explain_main(plans[i].fields, plans[i].n_terms, plans[i].mm, True)) for row, i in enumerate(picked)]


def edismax_search_batch(frame: pd.DataFrame,
                         queries: Sequence[str],
                         qf: List[str],
                         k: int = 10,
                         fq=None,
                         mm: Optional[Union[str, int]] = None,
                         pf: Optional[List[str]] = None,
                         pf2: Optional[List[str]] = None,
                         pf3: Optional[List[str]] = None,
                         ps2: int = 0,
                         ps3: int = 0,
                         ps: int = 0,
                         tie: float = 0.0,
                         q_op: str = "OR",
                         similarity: Union[Similarity, Dict[str, Similarity]] = default_bm25,
                         use_device: Optional[bool] = None) -> List[SearchHits]:
    """:func:`edismax_search` for a list of queries: ``hits[i]`` equals ``edismax_search(frame, queries[i], qf, k=k, fq=fq, ...)``
    field by field -- ``scores`` (dtype included), ``rows``, ``found``, ``explain``.  The other arguments are those of
    ``edismax_search`` and apply to every query; ``mm`` resolves against each query's own number of terms.

    Term-centric queries of 1 .. 32 terms are scored and ranked by ONE launch sequence over all of them (``FieldsBatch``: every
    (tile, query) item forms the float64 edismax score of its documents in LDS from the fields' postings, applies ``mm`` and
    ``fq`` and selects its best ``k``; a merge per query follows), with no per-row vector written for any query -- whenever the
    device route applies (``edismax``'s rule; ``use_device`` is not False), no ``pf`` / ``pf2`` / ``pf3`` is given and ``qf``
    names at most 8 fields.  Every other query -- field-centric ones, more than 32 terms -- or, when the condition is one of the
    call's, the whole list goes through ``edismax_search`` one by one and lands at its index; nothing raises because of the
    route and nothing differs.  An ``fq`` given as a mask or row ids becomes ONE device filter for the whole call, closed
    afterwards; a caller's ``DocFilter`` stays open.  ``k`` and ``fq`` are checked before anything is launched.

    Not covered: sharded frames (``devices=``), field-centric queries and phrase boosts on the batch kernel (they take the
    per-query route), bounds or pruning across tiles (every item scores its tile exhaustively), and the query-set queue."""
    k = int(k)
    if not 1 <= k <= 1024:
        raise ValueError("k must be in 1 .. 1024")
    queries = list(queries)
    plans = [_plan(frame, q, qf, mm, pf, pf2, pf3, q_op, similarity) for q in queries]
    n = len(frame)
    if isinstance(fq, DocFilter):
        if fq.index.n_docs != n:
            raise ValueError(f"fq covers {fq.index.n_docs} documents, the frame has {n} rows")
        mask = None
    else:
        mask = _fq_mask(frame, fq)                                  # (checked before anything is launched)
    if not plans:
        return []
    each = dict(k=k, mm=mm, pf=pf, pf2=pf2, pf3=pf3, ps2=ps2, ps3=ps3, ps=ps, tie=tie, q_op=q_op, similarity=similarity,
                use_device=use_device)
    fields = plans[0].fields                                        # (the fields are the call's; only their terms differ per query)
    device = _DeviceCombiner.usable(fields, n) if use_device is None else bool(use_device)
    if not device or not _DeviceCombiner.usable(fields, n):
        # the host route, or a forced device route on a frame the combiner cannot take: exactly what edismax_search does with it
        return [edismax_search(frame, q, qf, fq=fq if mask is None else mask, **each) for q in queries]
    own = None                                                      # ONE filter for the whole call, made here from a mask or row ids
    filt = fq
    if mask is not None:
        filt = own = fields[0].array._core.device().doc_filter(mask=mask)
    try:
        hits: List[Optional[SearchHits]] = [None] * len(queries)
        picked: List[int] = []
        if not (pf or pf2 or pf3) and len(fields) <= _BATCH_MAX_FIELDS:
            for i, plan in enumerate(plans):
                if plan.term_centric and all(len(f.terms) == plan.n_terms for f in plan.fields):
                    if plan.n_terms == 0:                           # no clause, no hit: what the empty device vector ranks to
                        hits[i] = SearchHits(np.zeros(k, dtype=np.float64), np.full(k, NO_DOC, dtype=np.uint64), 0,
                                             _explain_main(plan.fields, 0, plan.mm, True))
                    elif plan.n_terms <= _BATCH_MAX_TERMS:
                        picked.append(i)
        if picked:
            got = _fields_batch_hits(plans, picked, k, tie, filt)
            for i, h in zip(picked, got or []):
                hits[i] = h
        for i, q in enumerate(queries):
            if hits[i] is None:
                hits[i] = edismax_search(frame, q, qf, fq=filt, **each)
        return hits
    finally:
        if own is not None:
            own.close()


def _explain_main(fields: List[_Field], n_terms: int, mm: str, term_centric: bool) -> str:
    if term_centric:
        clauses = ["(" + " | ".join(f"{f.name}:{f.terms[p]}^{_boost_text(f.boost)}" for f in fields) + ")" for p in range(n_terms)]
        return "(" + " ".join(clauses) + f")~{parse_min_should_match(n_terms, spec=mm)}"
    texts = []
    for f in fields:
        need = min(parse_min_should_match(len(f.terms), spec=mm), len(f.terms))
        clause = " ".join(f"{f.name}:{t}" for t in f.terms)
        texts.append(f"(({clause})~{need})^{_boost_text(f.boost)}")
    return " | ".join(texts)


def _explain_phase(per_field, boosts, n) -> str:
    text = ""
    for field, boost in boosts.items():
        terms = per_field[field]
        if len(terms) < (2 if n is None else n):
            continue
        for gram in ([terms] if n is None else _ngrams(terms, n)):
            text += f" ({field}:\"{' '.join(gram)}\")^{_boost_text(boost)}"
    return text
