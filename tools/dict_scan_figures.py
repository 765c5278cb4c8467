"""Dictionary-scan time per probe (usage: python tools/dict_scan_figures.py): k_dict_scan / k_dict_scan_wide: 1 M-term dictionary (config #4's term count), 1024 distinct lev-2 probes per batch.
  bmp      all terms below U+10000, short probes           (k_dict_scan, the inline form)
  wide     10 % of the terms carry an emoji (u32 image)    (k_dict_scan_wide<u32>)
  long     BMP dictionary, probes of 100-200 code points   (k_dict_scan_wide<u16>, banded matcher) -- 2 % of the terms are long too"""
import json, os, random, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import veloci_amd
from veloci_amd.index import IndexData

ALPHA = "abcdefghijklmnopqrstuvwxyz"
EMOJI = ["🎉", "😀", "👍🏽", "𠮷", "𐐔"]


def make(kind, n_terms=1_000_000, seed=1):
    rng = random.Random(seed)
    words = set()
    while len(words) < n_terms:
        w = "".join(rng.choice(ALPHA) for _ in range(rng.randint(4, 12)))
        if kind == "wide" and rng.random() < 0.1:
            w = w[:rng.randint(0, len(w))] + rng.choice(EMOJI) + w[len(w) // 2:]
        if kind == "long" and rng.random() < 0.02:
            w = "".join(rng.choice(ALPHA[:6]) for _ in range(rng.randint(100, 200)))
        words.add(w)
    terms = sorted(w.encode() for w in words)
    T = len(terms)
    data = IndexData(100_000)
    offsets = np.arange(T + 1, dtype=np.uint64)
    anchors = (np.arange(T, dtype=np.uint32) * 7919) % 100_000
    data.add_fst("body.textindex", terms)
    data.add_token_to_anchor_score("body.textindex.to_anchor_id_score", offsets, anchors, np.full(T, 100, np.uint32), None)
    data.add_key_value_store("body.textindex.text_id_to_anchor", offsets, anchors)
    strs = [t.decode() for t in terms]
    if kind == "long":
        pool = [t for t in strs if len(t) >= 100]
    else:
        pool = strs
    probes = []
    for i in range(1024):
        s = list(rng.choice(pool))
        for _ in range(2):
            j = rng.randrange(len(s))
            s[j] = rng.choice(ALPHA)
        probes.append("".join(s))
    return data, probes


out = {}
for kind in ("bmp", "wide", "long"):
    data, probes = make(kind)
    idx = veloci_amd.Index(data, device=0)
    reqs = [{"search_req": {"search": {"path": "body", "terms": [p], "levenshtein_distance": 2}}, "top": 10} for p in probes]
    veloci_amd.search_batch(reqs, idx)  # warm-up
    idx.profile_enable(True)
    idx.profile_json(reset=True)
    reps = 5
    for _ in range(reps):
        veloci_amd.search_batch(reqs, idx)
    prof = idx.profile_json(reset=True)
    k = {n: v for n, v in prof.get("kernels", {}).items() if "dict" in n}
    ms = sum(v["ms"] for v in k.values()) / reps
    out[kind] = {"ms_per_batch": ms, "us_per_probe": 1e3 * ms / len(reqs), "raw": k}
    print(kind, json.dumps(out[kind]), flush=True)
    del idx
