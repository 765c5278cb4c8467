"""GPU parity of the probe kernels' LDS map on crafted posting lists: the unranked queue holds ONE round of 256 cover postings and is drained
early when a second round would not fit; an array operand's LDS slot is sized per launch by the fullest tile among the launch's array lists;
a list with a tile above 2048 entries is never an array operand.  Every answer against the CPU oracle, bit for bit.

The index spans 8 tiles of 32768 docs (262144 docs).  At that size a list has a bitmap image from 4096 postings on, a tile-packed image from
64 on, and is probed as a 16-bit array when it has no bitmap image or fewer than 16384 postings — as long as none of its tiles holds more
than 2048 entries.  The cover of an AND is its shortest list.  Each case first checks, on the CPU alone (numpy over the lists, hit counts
from the oracle), that the lists have the property the case is built for."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 8 * 32768
TILE = 32768
PATH = "body.textindex.to_anchor_id_score"
PROBE = "k_scan_probe (AND / OR)"


def every(step, lo=0, hi=N):
    return np.arange(lo, hi, step, dtype=np.int64)


def lists():
    far = np.concatenate([every(8, 0, TILE), every(8, 3 * TILE, N)])  # tiles 0 and 3..7: nothing in tiles 1 and 2
    run1 = np.arange(40000, 41000)                                     # 1000 consecutive docs inside tile 1
    L = {
        # ---- queue overflow: tile 1 holds 1000 cover postings that are in every operand, tile 2 holds 600 that are in none
        "c1": np.concatenate([run1, np.arange(70000, 70600)]),
        "b1": np.concatenate([run1, far]),                              # bitmap operand (25576 postings)
        "b2": np.concatenate([np.arange(39000, 42000), every(4, 4 * TILE, N)]),  # a second bitmap operand
        "a1": np.concatenate([run1, every(64, 0, TILE), every(64, 3 * TILE, 4 * TILE)]),  # array operand (2024 postings: no bitmap image)
        # ---- slot sizing: an array list with a clustered tile (1500 + 73 entries in tile 1) and one whose tiles are sparse (328 a tile)
        "c2": every(150),
        "ad": np.union1d(np.arange(33000, 34500), every(450)),
        "as": every(100),
        # ---- exclusion: 3000 entries in one tile — never an array; without a bitmap image (e1) not a probe operand at all
        "e1": np.arange(3 * TILE + 100, 3 * TILE + 3100),
        "e2": np.union1d(np.arange(3 * TILE + 100, 3 * TILE + 3100), every(100)),
    }
    return {k: np.unique(v).astype(np.uint32) for k, v in L.items()}


def per_tile(docs):
    return np.bincount(docs // TILE, minlength=N // TILE)


@pytest.fixture(scope="module")
def crafted():
    import veloci_amd
    from veloci_amd.index import IndexData
    from oracle import binding as O
    L = lists()
    terms = sorted(L)
    data = IndexData(N)
    data.add_fst("body.textindex", terms)
    data.set_column_meta("body", True, True)
    offsets = np.zeros(len(terms) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(L[t]) for t in terms])
    anchors = np.concatenate([L[t] for t in terms])
    scores = np.concatenate([1 + (L[t].astype(np.uint64) * (7 + 2 * i) % 1900) for i, t in enumerate(terms)]).astype(np.uint32)  # (integers below 2048: exact in f16)
    data.add_token_to_anchor_score(PATH, offsets, anchors, scores)
    ora = O.OracleIndex(N)
    data.load_into(ora)
    idx = veloci_amd.Index(data, device=0)
    idx.profile_enable(True)
    return L, idx, ora


def req_and(terms, top=10):
    return {"search_req": {"and": {"queries": [{"search": {"path": "body", "terms": [t]}} for t in terms]}}, "top": top}


def run(crafted, reqs, probe=True):
    """every request alone and all of them as one batch, against the oracle; -> the oracle's results.  probe: all / none of them ran on the probe kernels"""
    import veloci_amd
    from parity import assert_same
    L, idx, ora = crafted
    wants = [ora.search_json(json.dumps(r)) for r in reqs]
    for r, w in zip(reqs, wants):
        idx.profile_json(reset=True)
        assert_same(r, veloci_amd.search(r, idx), w)
        kernels = idx.profile_json(reset=True)["kernels"]
        assert (PROBE in kernels) == probe, (json.dumps(r), sorted(kernels))
        if probe:
            assert kernels[PROBE]["queries"] == 1 and not any(k.startswith("k_scan_simple") or k.startswith("k_tile_scan") for k in kernels), sorted(kernels)
    idx.profile_json(reset=True)
    for r, g, w in zip(reqs * 2, veloci_amd.search_batch(reqs * 2, idx), wants * 2):
        assert_same(r, g, w)
    kernels = idx.profile_json(reset=True)["kernels"]
    assert (PROBE in kernels) == probe and (not probe or kernels[PROBE]["queries"] == 2 * len(reqs)), sorted(kernels)
    return wants


def test_a_tile_with_more_hits_than_the_queue_holds(crafted):
    """1000 consecutive cover postings of one tile pass every operand: from the tile's second round on the unranked queue (256 entries) is full
    and is drained before the round's survivors are written — with an array operand (the lookups run early), with bitmap operands only (the
    ranking runs early), with one operand and with two.  The next tile holds 600 cover postings of which none passes."""
    L, idx, ora = crafted
    c1 = per_tile(L["c1"])
    assert c1[1] == 1000 and c1[2] == 600 and c1.sum() == 1600  # more than two rounds of 256 in tile 1
    for op in ("b1", "b2", "a1"):
        assert len(L["c1"]) < len(L[op])  # c1 is the cover
        assert np.isin(L["c1"][:1000], L[op]).all() and not np.isin(L["c1"][1000:], L[op]).any()
    assert len(L["b1"]) >= 16384 and len(L["b2"]) >= 16384       # bitmap operands
    assert 64 <= len(L["a1"]) < 4096 and per_tile(L["a1"]).max() <= 2048  # an array operand
    reqs = [req_and(["c1", "b1", "a1"]), req_and(["a1", "c1", "b1"], top=40), req_and(["c1", "a1"]), req_and(["c1", "b1"], top=3), req_and(["b2", "c1", "b1"]),
            req_and(["c1", "b1", "b2", "a1"], top=100), req_and(["c1", "a1", "b1"], top=1500)]
    wants = run(crafted, reqs)
    assert all(w.num_hits == 1000 for w in wants)


def test_the_array_slot_follows_the_fullest_tile_of_the_launch(crafted):
    """An array list with a tile of more than 1024 entries and one with sparse tiles: alone a launch sizes the operands' LDS slot by its own list,
    together by the fuller one; the answers are the same."""
    import veloci_amd
    from parity import assert_same
    L, idx, ora = crafted
    ad, as_ = per_tile(L["ad"]), per_tile(L["as"])
    assert 1025 <= ad.max() <= 2048 and len(L["ad"]) < 4096      # clustered, no bitmap image: probed as an array
    assert as_.max() <= 400 and 64 <= len(L["as"]) < 4096          # sparse
    assert len(L["c2"]) < min(len(L["ad"]), len(L["as"]))          # c2 is the cover
    dense = [req_and(["c2", "ad"]), req_and(["ad", "b2", "c2"], top=30), req_and(["c2", "ad", "as"], top=50)]
    sparse = [req_and(["c2", "as"]), req_and(["as", "c2", "b2"], top=30), req_and(["b1", "c2", "as"])]
    wd = run(crafted, dense)
    ws = run(crafted, sparse)
    assert all(w.num_hits > 0 for w in wd + ws)
    mixed = [r for pair in zip(dense, sparse) for r in pair]
    for r, g, w in zip(mixed, veloci_amd.search_batch(mixed, idx), [w for pair in zip(wd, ws) for w in pair]):
        assert_same(r, g, w)


def test_a_list_with_a_tile_above_2048_entries_is_no_array_operand(crafted):
    """3000 entries in one tile: with a bitmap image the list is probed as words, without one the AND runs on k_scan_simple — as before."""
    L, idx, ora = crafted
    assert per_tile(L["e1"]).max() == 3000 and len(L["e1"]) < 4096                 # no bitmap image, no array image
    assert per_tile(L["e2"]).max() > 2048 and 4096 <= len(L["e2"]) < 16384          # a bitmap image; short enough for an array if it had one
    assert len(L["c2"]) < len(L["e1"])
    wants = run(crafted, [req_and(["c2", "e2"]), req_and(["c2", "e2", "as"], top=20)], probe=True)
    wants += run(crafted, [req_and(["c2", "e1"]), req_and(["c2", "as", "e1"], top=20)], probe=False)
    assert all(w.num_hits > 0 for w in wants)
