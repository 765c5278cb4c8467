"""Doc sets restated in numpy: the image a DocSet must hold (tests/test_gpu_docset.py on the device, tests/test_docset_cpu.py over the stubbed
device layer), the id lists both tests build their sets from, and a small index to build them on."""
import numpy as np

NUM_ANCHORS = 200_003  # no multiple of 32, 512 or 16384
SHARD = (70_001, 150_000)  # not aligned to 65536: the bitmap base (65536) lies below doc_lo


def image(ids, num_anchors, doc_lo, doc_hi):
    """-> dict: len, local_len, docs, padded, bitmap / rank_dir / tile_dir (None: the set carries no such part), device_bytes"""
    u = np.unique(np.asarray(ids, np.int64))
    assert u.size == 0 or (u[0] >= 0 and u[-1] < num_anchors)
    local = u[(u >= doc_lo) & (u < doc_hi)]
    base = doc_lo & ~65535
    words = (doc_hi - base + 65535) // 65536 * 2048 + 2048  # [base, doc_hi) in whole 65536-doc pieces and one tile of slack
    blocks, tiles = words // 16, words // 512 + 3
    span = doc_hi - doc_lo
    dense = span >= 65536 and local.size * 64 >= span
    tiled = span >= 65536 and local.size * 4096 >= span
    rel = local - base
    bits = np.zeros(words * 32, np.uint8)
    bits[rel] = 1
    bitmap = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
    rank = np.concatenate([[0], np.cumsum(np.bincount(rel >> 9, minlength=blocks))]).astype(np.uint32)  # entries below base + 512 k
    tile = np.concatenate([[0], np.cumsum(np.bincount(rel >> 14, minlength=tiles))]).astype(np.uint32)  # entries below base + 16384 k
    assert rank.size == blocks + 1 and tile.size == tiles + 1
    padded = np.concatenate([local, np.full(-local.size % 4, 0xFFFFFFFF)]).astype(np.uint32)
    nbytes = padded.size * 4 + 16
    if dense:
        nbytes += words * 4 + 16 + (blocks + 1) * 4 + 16
    if tiled:
        nbytes += (tiles + 1) * 4 + 16
    return {"len": int(u.size), "local_len": int(local.size), "docs": local.astype(np.uint32), "padded": padded, "bitmap": bitmap if dense else None,
            "rank_dir": rank if dense else None, "tile_dir": tile if tiled else None, "device_bytes": nbytes, "base": base}


def id_lists(num_anchors=NUM_ANCHORS, seed=5):
    """name -> ids (numpy int64, any order, duplicates where the name says so)"""
    rng = np.random.default_rng(seed)
    edges = np.array([0, 31, 32, 511, 512, 16383, 16384, 32767, 32768, 65535, 65536])
    once = rng.choice(num_anchors, size=3000, replace=False)
    return {
        "empty": np.zeros(0, np.int64),
        "one": np.array([77_777]),
        "last": np.array([num_anchors - 1]),
        "every": np.arange(num_anchors),
        "edges": edges,
        "repeated": rng.permutation(np.repeat(once, rng.integers(1, 6, size=once.size))),
        "sparse": rng.choice(num_anchors, size=200, replace=False),
        "medium": rng.choice(num_anchors, size=6000, replace=False),
        "dense": rng.choice(num_anchors, size=80_000, replace=False),
    }


def check(ds, ids, num_anchors, doc_lo, doc_hi):
    """every part of DocSet `ds` against the restatement, element for element"""
    want = image(ids, num_anchors, doc_lo, doc_hi)
    assert len(ds) == want["len"] and ds.local_len == want["local_len"], (len(ds), ds.local_len, want["len"], want["local_len"])
    assert np.array_equal(ds.ids(), want["docs"])
    assert np.array_equal(ds.part(4), want["padded"])
    for which, name in ((1, "bitmap"), (2, "rank_dir"), (3, "tile_dir")):
        got = ds.part(which)
        if want[name] is None:
            assert got.size == 0, (name, got.size)
        else:
            assert got.size == want[name].size and np.array_equal(got, want[name]), (name, got.size, want[name].size, np.flatnonzero(got != want[name][:got.size])[:5])
    assert ds.device_bytes == want["device_bytes"], (ds.device_bytes, want["device_bytes"])
    return want


def small_data(num_anchors=NUM_ANCHORS):
    """an index with one two-term field: all a doc set needs of its index is the doc range"""
    import veloci_amd
    data = veloci_amd.IndexData(num_anchors)
    offsets = np.array([0, 3, 5], np.uint64)
    anchors = np.array([1, 70_500, 149_000, 2, 100_000], np.uint32)
    data.add_fst("body.textindex", [b"alpha", b"beta"])
    data.add_token_to_anchor_score("body.textindex.to_anchor_id_score", offsets, anchors, np.full(5, 10, np.uint32), None)
    data.add_key_value_store("body.textindex.text_id_to_anchor", offsets, anchors)
    data.set_column_meta("body", False, True)
    return data
