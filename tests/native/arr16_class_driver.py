"""Driver of the host-stub build for the probe kernels' 16-bit array images (run by tests/test_arr16_class_cpu.py with VQ_LIB=<host-stub library>):
crafted lists are staged over the stubbed device layer, read back through vq_debug_arr16_list and checked entry by entry — sorted tiles, pads
0xFFFF, no real entry 0xFFFF, the class bit set exactly where the posting's raw f16 score is <= the list's pivot (never at in-tile offset 32767),
the pivot by the quantile rule."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import veloci_amd  # noqa: E402
from veloci_amd import _lib  # noqa: E402
from veloci_amd.index import IndexData  # noqa: E402

assert "host_" in _lib.lib_path(), _lib.lib_path()
TILE = 32768
N = 5 * TILE + 777
PATH = "body.textindex.to_anchor_id_score"
DIV = 8  # device_types.hpp: kScoreClassDiv

rng = np.random.default_rng(7)
ends = np.array([1 * TILE + 32767, 2 * TILE + 32767, 3 * TILE + 32767])
base = np.arange(0, N, 20)
LISTS = {
    "equal": (base, np.full(len(base), 700)),                                                  # no class
    "graded": (np.union1d(base, ends), None),                                                  # 40 values; offsets 32767 with a low, the pivot's and a high score
    "twoval": (base, np.where(np.arange(len(base)) % 10 == 0, 1500, 300)),                     # a tenth on top: fewer than 1/8 lie above 300 — no value of the list qualifies
    "topheavy": (base, np.where(np.arange(len(base)) % 3 == 0, 1500, 300)),                    # a third on top: the pivot is the lower value
    "inf": (base, np.where(np.arange(len(base)) == 5, 70000, 1 + np.arange(len(base)) % 900)),  # 70000 is +inf in f16: not all finite, no class
    "dense": (np.arange(0, N, 2), None),                                                       # more than 2048 entries a tile: no array image
    "tiny": (np.arange(0, N, 9000), None),                                                     # below 1/4096 of the docs: no tile-packed image
}
for t in ("graded", "dense", "tiny"):
    d = LISTS[t][0]
    LISTS[t] = (d, 100 + rng.integers(0, 40, len(d)) * 25)
d, s = LISTS["graded"]
s[d == ends[0]], s[d == ends[2]] = 100, 1075

terms = sorted(LISTS)
data = IndexData(N)
data.add_fst("body.textindex", terms)
data.set_column_meta("body", True, True)
offsets = np.zeros(len(terms) + 1, np.uint64)
offsets[1:] = np.cumsum([len(LISTS[t][0]) for t in terms])
data.add_token_to_anchor_score(PATH, offsets, np.concatenate([LISTS[t][0] for t in terms]).astype(np.uint32), np.concatenate([LISTS[t][1] for t in terms]).astype(np.uint32))
idx = veloci_amd.Index(data, device=0)
f = idx.L.vq_debug_arr16_list
f.restype = C.c_uint64
f.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]


def image(token):
    pivot, most = C.c_uint16(0), C.c_uint16(0)
    n = int(f(idx.h, PATH.encode(), token, None, 0, C.byref(pivot), C.byref(most)))
    out = np.zeros(n, np.uint16)
    if n:
        assert int(f(idx.h, PATH.encode(), token, out.ctypes.data_as(C.c_void_p), n, C.byref(pivot), C.byref(most))) == n
    return out, pivot.value, most.value


seen_end_low = False
for token, t in enumerate(terms):
    docs, scores = LISTS[t]
    raw = scores.astype(np.float32).astype(np.float16).view(np.uint16)
    arr, pivot, most = image(token)
    if t in ("dense", "tiny"):
        assert len(arr) == 0, t
        continue
    assert most == raw.max(), t
    # the quantile rule: the largest raw value of the list that at least ceil(len / DIV) raw scores lie above; none (or a score that is not finite): the maximum
    need = (len(raw) + DIV - 1) // DIV
    want = max((int(r) for r in np.unique(raw) if np.count_nonzero(raw > r) >= need), default=int(most)) if most < 0x7C00 else int(most)
    assert pivot == want, (t, pivot, want)
    assert (pivot == most) == (t in ("equal", "twoval", "inf")), (t, pivot, most)
    classed = pivot < most
    at = 0
    for k in range(N // TILE + 1):
        sel = docs // TILE == k
        cnt = int(sel.sum())
        padded = (cnt + 7) // 8 * 8
        tile = arr[at:at + padded].astype(np.uint32)
        at += padded
        assert (np.diff(tile.astype(np.int64)) >= 0).all(), (t, k)            # sorted, the pads last
        assert (tile[cnt:] == 0xFFFF).all() and (tile[:cnt] != 0xFFFF).all(), (t, k)
        rel = (docs[sel] - k * TILE).astype(np.uint32)
        assert (tile[:cnt] >> 1 == rel).all(), (t, k)
        low = classed & (raw[sel] <= pivot) & (rel != 32767)
        assert ((tile[:cnt] & 1) == low).all(), (t, k)
        seen_end_low |= bool(classed and ((rel == 32767) & (raw[sel] <= pivot)).any())
    assert at == len(arr) or (arr[at:] == 0xFFFF).all(), t
assert seen_end_low  # a low-class posting at offset 32767 occurred (and was written without the bit)
print("ARR16_CLASS_DRIVER_OK")
