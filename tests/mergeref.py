"""The two merges every search ends in (k_merge_spans, k_finalize), restated plainly in numpy: a top-k over unique non-zero u64 keys.
A ranking key is (order_f32(score bits) << 32) | doc id, larger = better under (score descending, id descending); 0 is an empty slot.
Inputs hold unique non-zero keys beside the zeros: the product's keys come from disjoint doc ranges."""
import numpy as np


def order_f32(bits):
    """f32 bit patterns -> u32 words that order like the floats (device_types.hpp)"""
    bits = np.asarray(bits, np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def unorder_f32(words):
    words = np.asarray(words, np.uint32)
    return np.where(words & np.uint32(0x80000000), words & np.uint32(0x7FFFFFFF), ~words).astype(np.uint32)


def make_key(score_f32, doc):
    """-> u64 keys of (f32 score, doc id) pairs"""
    bits = np.asarray(score_f32, np.float32).view(np.uint32)
    return (order_f32(bits).astype(np.uint64) << np.uint64(32)) | np.asarray(doc, np.uint64)


def merge_ref(keys, top_k):
    """the non-zero keys, sorted descending as u64, the first top_k, zero-padded to top_k"""
    keys = np.asarray(keys, np.uint64).ravel()
    best = np.sort(keys[keys != 0])[::-1][:top_k]
    out = np.zeros(top_k, np.uint64)
    out[:len(best)] = best
    return out


def finalize_ref(shard_keys, shard_hits, top_k):
    """shard_keys: the shards' key lists (any shape), shard_hits: one count per shard -> (ids[n], score bits[n], n, hits)"""
    window = merge_ref(np.concatenate([np.asarray(k, np.uint64).ravel() for k in shard_keys]), top_k)
    n = int(np.count_nonzero(window))
    ids = (window[:n] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    score_bits = unorder_f32((window[:n] >> np.uint64(32)).astype(np.uint32))
    hits = 0
    for h in shard_hits:
        hits = (hits + int(h)) & 0xFFFFFFFFFFFFFFFF  # a u64 sum
    return ids, score_bits, n, hits
