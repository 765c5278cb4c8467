"""Per-kernel device time of the union step, dense route against k_union: usage  python tools/measure_union_dense.py LABEL [scale] [config4]
(VQ_UNION_DENSE_MIN is read once per process: run once with the default and once with 1).  Writes profiles/union_dense/LABEL.json."""
import json, os, re, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import veloci_amd, widecorpus
from veloci_amd import synth

label, what = sys.argv[1], sys.argv[2:]
out = {"label": label, "VQ_UNION_DENSE_MIN": os.environ.get("VQ_UNION_DENSE_MIN", "(default 4096)"), "legs": []}
UK = ("k_union<count>", "k_union<write>", "k_union_dense_scatter", "k_union_dense_count", "k_union_dense_write", "k_dict_scan")

def leg(name, idx, reqs, reps, batch=False, extra=None):
    run = (lambda: veloci_amd.search_batch(reqs, idx)) if batch else (lambda: [veloci_amd.search(r, idx) for r in reqs])
    for _ in range(3):
        res = run()
    idx.profile_enable(); idx.profile_json()
    t0 = time.perf_counter()
    for _ in range(reps):
        res = run()
    wall = (time.perf_counter() - t0) / reps
    prof = idx.profile_json()
    idx.profile_enable(False)
    row = {"leg": name, "reps": reps, "requests": len(reqs), "batched": batch, "wall_ms_per_rep": wall * 1e3, "num_hits": [int(r.num_hits) for r in res][:8],
           "per_rep": {k: {"ms": v["ms"] / reps, "launches": v["launches"] / reps, "layout_bytes": v["layout_bytes"] / reps, "algorithmic_bytes": v["algorithmic_bytes"] / reps, "jobs": v["queries"] / reps}
                       for k, v in prof["kernels"].items() if k in UK},
           "profile_json": prof}
    if extra: row.update(extra)
    out["legs"].append(row)
    print(name, json.dumps(row["per_rep"]), flush=True)

def pre(t, **kw): return {"search_req": {"search": dict({"path": "body", "terms": [t], "starts_with": True}, **kw)}, "top": 10}

data, terms = widecorpus.build(num_terms=40_000, num_docs=1_000_000)
idx = veloci_amd.Index(data, device=0)
cnt = lambda p: sum(1 for t in terms if t.startswith(p.encode()))
rx = "zr[a-f].*"
n_rx = sum(1 for t in terms if re.fullmatch("[\\s\\S]*?(?:" + rx + ")", t.decode()))
two = sorted((abs(cnt("a" + c) - 256), "a" + c) for c in "abcdefghijklmnopqrstuvwxyz")[0][1]
for name, req, n in ((two, pre(two), cnt(two)), ("regex " + rx, {"search_req": {"search": {"path": "body", "terms": [rx], "is_regex": True}}, "top": 10}, n_rx),
                     ("zrc", pre("zrc"), cnt("zrc")), ("zr", pre("zr"), cnt("zr")), ("zq", pre("zq"), cnt("zq")), ("a", pre("a"), cnt("a"))):
    leg("40k corpus, 1 M docs: %s (%d lists)" % (name, n), idx, [req], 20, extra={"lists": n})
del idx

if "scale" in what:
    for N in (1_000_000, 10_000_000):
        data, terms = widecorpus.build(num_terms=300_000, num_docs=N, planted=False)
        idx = veloci_amd.Index(data, device=0)
        n = sum(1 for t in terms if t.startswith(b"a"))
        leg("300k corpus, %d docs: a (%d lists)" % (N, n), idx, [pre("a")], 20, extra={"lists": n, "docs": N})
        leg("300k corpus, %d docs: a, b, c, d in one batch" % N, idx, [pre(c) for c in "abcd"], 10, batch=True, extra={"docs": N})
        del idx

if "config4" in what:
    import bench
    spec = synth.SynthSpec(num_docs=10_000_000, num_terms=1_000_000, triples=4, with_t2t=False, with_phrase=False, with_boost=False, with_facets=True, background_terms=2000)
    data, meta = synth.generate(spec)
    idx = veloci_amd.Index(data, device=0)
    pool = [t for tr in meta.triples for t in tr] + list(meta.background)
    qterms = bench.edited_terms(pool, 100)
    reqs = [{"search_req": {"search": {"path": "body", "terms": [t], "levenshtein_distance": 2}}, "top": 10, "facets": [{"field": "cat"}, {"field": "tags[]"}]} for t in qterms]
    leg("config #4 shape: 10 M docs, 1 M terms, 100 lev-2 requests in one batch", idx, reqs, 10, batch=True)
    del idx

os.makedirs(os.path.join(ROOT, "profiles", "union_dense"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "union_dense", label + ".json"), "w") as f:
    json.dump(out, f, indent=1)
print("MEASURE_OK", label)
