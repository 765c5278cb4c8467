"""Plain restatements of what the pre-pass drivers build (prepass.cpp run_union_jobs / run_locality_jobs / run_range_jobs / run_boost1n_jobs), over the
raw arrays an IndexData was filled from.  Loops and numpy float32 only; tests/test_gpu_prepass_lists.py compares every entry of the device lists
with these, tests/test_prepass_ref_cpu.py pins them against the CPU oracle.

Stores are the tuples IndexData keeps: postings (offsets, anchors, scores, _), key-value stores (key_base, offsets, values), boost columns
(key_base, present | None, value_bits)."""
import numpy as np


def _row(store, key):
    """IndexIdToParent::get_values: the row of `key`, empty outside the key range"""
    key_base, offsets, values = store
    r = int(key) - key_base
    if r < 0 or r >= len(offsets) - 1:
        return values[:0]
    return values[int(offsets[r]):int(offsets[r + 1])]


def union(postings, tokens, term_scores, doc_lo=0, doc_hi=None):
    """-> (docs u32 ascending, values f32, max_value f32): per doc the largest term_score * (f16 score / 100) over the lists `tokens`"""
    offsets, anchors, scores = postings[0], postings[1], postings[2]
    best = {}
    for t, ts in zip(tokens, term_scores):
        row = slice(int(offsets[t]), int(offsets[t + 1]))
        f16 = scores[row].astype(np.float32).astype(np.float16)  # the stored integer score as the loader keeps it: f16, round to nearest even
        vals = np.float32(ts) * (f16.astype(np.float32) / np.float32(100))
        for d, v in zip(anchors[row].tolist(), vals):
            if d < doc_lo or (doc_hi is not None and d >= doc_hi):
                continue
            if d not in best or v > best[d]:
                best[d] = v
    docs = np.array(sorted(best), np.uint32)
    vals = np.array([best[int(d)] for d in docs], np.float32)
    return docs, vals, (vals.max() if len(vals) else np.float32(0.0))


def locality(t2t, t2a, tokens, doc_lo=0, doc_hi=None):
    """-> (anchors u32 ascending, values f32): texts that occur c > 1 times in the rows of `tokens` give each of their anchors 2 * c * c;
    the smallest value per anchor"""
    count = {}
    for t in tokens:
        for text in _row(t2t, t):
            count[int(text)] = count.get(int(text), 0) + 1
    best = {}
    for text, c in count.items():
        if c <= 1:
            continue
        v = np.float32(2) * np.float32(c) * np.float32(c)
        for a in _row(t2a, text):
            a = int(a)
            if a < doc_lo or (doc_hi is not None and a >= doc_hi):
                continue
            if a not in best or v < best[a]:
                best[a] = v
    docs = np.array(sorted(best), np.uint32)
    return docs, np.array([best[int(d)] for d in docs], np.float32)


def range_hits(postings, tokens, anchors):
    """-> counts u64 [2 * len(anchors)]: [2j] postings equal to a_j, [2j + 1] postings strictly between a_(j-1) and a_j (0 for j = 0)"""
    offsets, docs = postings[0], postings[1]
    counts = np.zeros(2 * len(anchors), np.uint64)
    for t in tokens:
        row = docs[int(offsets[t]):int(offsets[t + 1])]
        for j, a in enumerate(anchors):
            counts[2 * j] += int(np.count_nonzero(row == a))
            if j:
                counts[2 * j + 1] += int(np.count_nonzero((row > anchors[j - 1]) & (row < a)))
    return counts


def boost1n(to_parent, to_anchor, boost, text_ids, doc_lo=0, doc_hi=None):
    """-> (anchors u32, value bits u32, total, ascending, several): the value ids of `text_ids`, sorted with duplicates, each one that both
    tables know, that has a boost value and a non-empty anchor row mapped to (first anchor of the row, boost value); the list is the part inside
    [doc_lo, doc_hi), total / ascending / several speak of all kept pairs"""
    vids = sorted(int(v) for t in text_ids for v in _row(to_parent, t))
    b_base, present, bits = boost
    kept = []
    for v in vids:
        r = v - b_base
        if r < 0 or r >= len(bits) or (present is not None and not present[r]):
            continue
        row = _row(to_anchor, v)
        if len(row):
            kept.append((int(row[0]), int(bits[r])))
    ascending = all(kept[i][0] >= kept[i - 1][0] for i in range(1, len(kept)))
    several = any(kept[i][0] == kept[i - 1][0] for i in range(1, len(kept)))
    mine = [(a, b) for a, b in kept if a >= doc_lo and (doc_hi is None or a < doc_hi)]
    return (np.array([a for a, _ in mine], np.uint32), np.array([b for _, b in mine], np.uint32), len(kept), ascending, several)
