"""Indexes from raw arrays for the pre-pass kernels (tests/test_gpu_prepass_lists.py) and thin callers of the vq_debug_*_lists entry points.
widecorpus.crafted builds posting lists from (term, docs); here the key-value stores and boost columns of the text-locality and 1:n-boost
pre-passes are crafted as well, under the path names that make the loader stage the device images the drivers read."""
import ctypes as C

import numpy as np

from veloci_amd.index import IndexData, csr_from_lists

POSTINGS = "body.textindex.to_anchor_id_score"
PAD = 8
CAP = 1 << 21  # entries of the callers' output arrays


def postings_data(num_docs, lists):
    """lists: [(docs ascending unique, integer scores)] -> IndexData with the lists as tokens 0 .. len(lists) - 1 of POSTINGS"""
    data = IndexData(num_docs)
    off, docs = csr_from_lists([d for d, _ in lists])
    _, scores = csr_from_lists([s for _, s in lists])
    assert len(docs) == len(scores)
    data.add_fst("body.textindex", ["t%06d" % i for i in range(len(lists))])
    data.add_token_to_anchor_score(POSTINGS, off, docs, scores, None)
    return data


class KVBuilder:
    """rows of one key-value store, appended one by one: add(row) -> key"""

    def __init__(self, key_base=0):
        self.key_base = key_base
        self.rows = []

    def add(self, row):
        self.rows.append(np.asarray(row, np.uint32))
        return self.key_base + len(self.rows) - 1

    def store(self):
        off, vals = csr_from_lists(self.rows)
        return off, vals


def rows_for_counts(t2t, counts):
    """counts: {text id: c}.  Appends max(c) token rows to `t2t`, row k = the texts with c > k, and returns their token ids: gathered together they hold
    every text c times."""
    top = max(counts.values(), default=0)
    return [t2t.add(sorted(t for t, c in counts.items() if c > k)) for k in range(top)]


# ---- callers -------------------------------------------------------------------------------------------------------------------------------

def _paths(paths):
    return (C.c_char_p * len(paths))(*[p.encode() for p in paths])


def _csr(jobs):
    off = np.zeros(len(jobs) + 1, np.uint64)
    off[1:] = np.cumsum([len(j) for j in jobs], dtype=np.uint64)
    flat = np.concatenate([np.asarray(j, np.uint32) for j in jobs]) if int(off[-1]) else np.zeros(0, np.uint32)
    return off, np.ascontiguousarray(flat, np.uint32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _split(lens, docs, bits):
    out, at = [], 0
    for n in lens:
        n = int(n)
        out.append((docs[at:at + n + PAD].copy(), bits[at:at + n + PAD].copy()))
        at += n + PAD
    return out


def run_union(idx, jobs, route, cap=CAP, path=POSTINGS, paths=None):
    """jobs: [(tokens, term scores f32)] -> (rc, [(docs[len + 8], value bits[len + 8], max bits)])"""
    off, tokens = _csr([t for t, _ in jobs])
    scores = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float32) for _, s in jobs]) if len(tokens) else np.zeros(0, np.float32)).view(np.uint32)
    n = len(jobs)
    lens, maxes = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    docs, bits = np.full(cap, 0xDEAD, np.uint32), np.full(cap, 0xDEAD, np.uint32)
    rc = idx.L.vq_debug_union_lists(idx.h, _paths(paths or [path] * n), _p(off), _p(tokens), _p(scores), n, route, cap, _p(lens), _p(maxes), _p(docs), _p(bits))
    if rc != 0:
        return rc, None
    return rc, [(d, b, int(m)) for (d, b), m in zip(_split(lens, docs, bits), maxes)]


def run_locality(idx, jobs, cap=CAP):
    """jobs: [(tokens_to_text_id path, text_id_to_anchor path, tokens)] -> (rc, [(docs[len + 8], value bits[len + 8])])"""
    off, tokens = _csr([t for _, _, t in jobs])
    n = len(jobs)
    lens = np.zeros(n, np.uint32)
    docs, bits = np.full(cap, 0xDEAD, np.uint32), np.full(cap, 0xDEAD, np.uint32)
    rc = idx.L.vq_debug_locality_lists(idx.h, _paths([a for a, _, _ in jobs]), _paths([b for _, b, _ in jobs]), _p(off), _p(tokens), n, cap, _p(lens), _p(docs), _p(bits))
    return rc, (_split(lens, docs, bits) if rc == 0 else None)


def run_range_hits(idx, jobs, path=POSTINGS):
    """jobs: [(tokens, ascending anchors)] -> (rc, [counts u64 [2 * anchors]])"""
    toff, tokens = _csr([t for t, _ in jobs])
    aoff, anchors = _csr([a for _, a in jobs])
    counts = np.full(2 * len(anchors) + 1, 0xDEAD, np.uint64)
    rc = idx.L.vq_debug_range_hits(idx.h, _paths([path] * len(jobs)), _p(toff), _p(tokens), _p(aoff), _p(anchors), len(jobs), _p(counts))
    if rc != 0:
        return rc, None
    return rc, [counts[2 * int(aoff[j]):2 * int(aoff[j + 1])].copy() for j in range(len(jobs))]


def run_boost1n(idx, jobs, cap=CAP):
    """jobs: [(value_id_to_parent path, value_id_to_anchor path, boost path, text ids)] -> (rc, [(docs[len + 8], value bits[len + 8], total, ascending, several)])"""
    off, texts = _csr([t for _, _, _, t in jobs])
    n = len(jobs)
    lens, totals, flags = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    docs, bits = np.full(cap, 0xDEAD, np.uint32), np.full(cap, 0xDEAD, np.uint32)
    rc = idx.L.vq_debug_boost1n_lists(idx.h, _paths([j[0] for j in jobs]), _paths([j[1] for j in jobs]), _paths([j[2] for j in jobs]), _p(off), _p(texts), n, cap,
                                      _p(lens), _p(totals), _p(flags), _p(docs), _p(bits))
    if rc != 0:
        return rc, None
    return rc, [(d, b, int(t), bool(f & 1), bool(f & 2)) for (d, b), t, f in zip(_split(lens, docs, bits), totals, flags)]
