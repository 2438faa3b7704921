"""The two-field frame (`title`, `body`) of the edismax benchmarks (scripts/edismax_bench.py, scripts/edismax_batch_bench.py): seeded
Zipf documents over 50 000 tokens `t0 ... t49999`, titles a quarter as long as bodies.  from_tokens builds the columns from the token
ids directly (the index is encoded on the device, no Python strings: what makes 10 M docs practical; the documents are the same)."""
import numpy as np
import pandas as pd

from searcharray_amd import SearchArray, synth

VOCAB = 50_000
NAMES = np.array([f"t{i}" for i in range(VOCAB)])


def array_from_tokens(lens, terms, starts):
    """the SearchArray that SearchArray.index builds from the joined strings, from the token ids themselves"""
    from searcharray_amd.indexing import HostIndex
    from searcharray_amd.postings import _IndexCore, ws_tokenizer
    from searcharray_amd.term_dict import TermDict
    present = np.unique(terms)                                   # (index() numbers the terms in order of first appearance; ids are
    term_dict = TermDict()                                       #  internal, so any numbering gives the same scores)
    term_dict.add_terms([str(t) for t in NAMES[present]])
    remap = np.zeros(VOCAB, dtype=np.uint32)
    remap[present] = np.arange(len(present), dtype=np.uint32)
    host = HostIndex(term_dict, lens.astype(np.float32), tokens=np.ascontiguousarray(remap[terms]),
                     doc_ptr=np.ascontiguousarray(starts, dtype=np.uint64))
    arr = SearchArray.__new__(SearchArray)
    arr.avoid_copies, arr.tokenizer, arr._core, arr._rows = True, ws_tokenizer, _IndexCore(host), None
    return arr


def build_frame(docs: int, from_tokens: bool) -> pd.DataFrame:
    frames = {}
    for field, seed_off in (("title", 0), ("body", 1)):
        lens, terms = synth.zipf_batch_tokens(seed_off, docs, VOCAB, fast=True)
        if field == "title":
            lens = np.maximum(1, lens // 4)
            starts = np.concatenate([[0], np.cumsum(lens)])
            terms = terms[:starts[-1]]
        starts = np.concatenate([[0], np.cumsum(lens)])
        if from_tokens:
            frames[field] = array_from_tokens(lens, terms[:starts[-1]], starts)
        else:
            frames[field] = SearchArray.index([" ".join(NAMES[terms[starts[i]:starts[i + 1]]]) for i in range(docs)])
    return pd.DataFrame(frames)
