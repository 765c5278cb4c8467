"""Doc sets from a filter tree on the bench index (profiles/docset_filter/README.md holds the results):

  construction   DocSet.from_filter of four trees over the rows of an `acl` field (one dense leaf, an OR of 8 leaves of mixed density, a depth-3
                 tree, a one-letter prefix): the HIP event time of the evaluation (VQ_DOCSET_TIMING=1: the "mark" slot is k_filter_bits) and the
                 wall time of the call, after --warmup, --repeats times each, next to the bytes the evaluation must move (4 B per id of every list
                 it reads, range / 8 written) and their share of the HBM peak
  use            a --batch-request step of 3-term ANDs (the bench's triples) under `filter: T`, T = AND(acl row, OR of two rows), against the same
                 step under DocSet.from_filter(T), through vq_search_batch_flat.  The two forms alternate, --repeats timed steps each after
                 --warmup; the filter form's own spread is the noise.  The first step's rows of the two forms are compared: they must be the same.
                 One profiled step each names the kernels that ran.

usage: python tools/docset_filter_bench.py [--docs 100000000] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("VQ_DOCSET_TIMING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12  # B/s, MI355X

# the rows of the `acl` field: name -> share of the docs
ROWS = [("g0", 0.01), ("g1", 0.30),
        ("h0", 0.0001), ("h1", 0.001), ("h2", 0.01), ("h3", 0.03), ("h4", 0.05), ("h5", 0.10), ("h6", 0.005), ("h7", 0.0005),
        ("p0", 0.001), ("p1", 0.001), ("p2", 0.001), ("p3", 0.001), ("p4", 0.001), ("p5", 0.001)]


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def leaf(term, **kw):
    return {"search": dict({"path": "acl", "terms": [term]}, **kw)}


def AND(*qs):
    return {"and": {"queries": list(qs)}}


def OR(*qs):
    return {"or": {"queries": list(qs)}}


def lists_read(tree):
    """the acl rows a tree reads, one entry per leaf occurrence (a prefix leaf: every row it matches)"""
    if "search" in tree:
        part = tree["search"]
        return [n for n, _ in ROWS if n.startswith(part["terms"][0])] if part.get("starts_with") else [part["terms"][0]]
    return [n for q in tree["and" if "and" in tree else "or"]["queries"] for n in lists_read(q)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--terms", type=int, default=100_000)
    ap.add_argument("--triples", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import veloci_amd
    from veloci_amd import synth

    t0 = time.time()
    data, meta = synth.generate(synth.SynthSpec(num_docs=args.docs, num_terms=args.terms, triples=args.triples, with_t2t=False, with_facets=False, with_boost=False,
                                                with_phrase=False), device="cuda:0")
    rng = np.random.default_rng(3)
    order = sorted(range(len(ROWS)), key=lambda k: ROWS[k][0])  # dictionary order
    rows = {ROWS[k][0]: np.flatnonzero(rng.random(args.docs) < ROWS[k][1]).astype(np.uint32) for k in order}
    names = [ROWS[k][0] for k in order]
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(rows[n]) for n in names])
    data.add_fst("acl.textindex", [n.encode() for n in names])
    data.add_key_value_store("acl.textindex.text_id_to_anchor", off, np.concatenate([rows[n] for n in names]))
    index = veloci_amd.Index(data, device=0)
    out = {"docs": args.docs, "batch": args.batch, "build_s": round(time.time() - t0, 1), "rows": {n: int(len(rows[n])) for n in names}, "construction": [], "use": []}
    print(f"index: {args.docs} docs, {index.device_bytes / 1e9:.2f} GB, {out['build_s']} s", flush=True)

    # ---- construction
    cases = [("dense leaf", leaf("g1")),
             ("or of 8 leaves", OR(*[leaf("h%d" % k) for k in range(8)])),
             ("depth-3 tree", AND(OR(AND(leaf("h5"), leaf("g1")), leaf("h2")), OR(leaf("h3"), AND(leaf("h4"), leaf("h5"))), leaf("g1"))),
             ("one-letter prefix", leaf("p", starts_with=True))]
    for name, tree in cases:
        ev, wall = [], []
        for it in range(args.warmup + args.repeats):
            t = time.perf_counter()
            ds = veloci_amd.DocSet.from_filter(index, tree)
            w = (time.perf_counter() - t) * 1e3
            tm = ds.timings()
            n_ids, nbytes = len(ds), ds.device_bytes
            ds.close()
            if it >= args.warmup:
                ev.append(tm[0]), wall.append(w)
        read = sum(4 * len(rows[n]) for n in lists_read(tree))
        if name == "one-letter prefix":  # more than four rows in one leaf: united on the host, the kernel reads the united list
            read = 4 * n_ids
        written = args.docs // 8
        e = stats(ev)
        row = {"case": name, "tree": tree, "ids": n_ids, "device_bytes": nbytes, "evaluate_ms": e, "call_wall_ms": stats(wall), "bytes_read": read, "bytes_written": written,
               "share_of_hbm_peak": round((read + written) / (e["median"] * 1e-3) / HBM_PEAK, 4)}
        out["construction"].append(row)
        print(json.dumps(row), flush=True)

    # ---- a step under the tree as `filter`, against the same step under the set made from it
    T = AND(leaf("g1"), OR(leaf("h2"), leaf("h3")))
    reqs = [synth.req_and(list(meta.triples[i % len(meta.triples)]), top=10) for i in range(args.batch)]
    ds = veloci_amd.DocSet.from_filter(index, T)
    forms = {"set": veloci_amd.RequestBatch(reqs, docsets=[ds] * len(reqs)), "filter": veloci_amd.RequestBatch([dict(r, filter=T) for r in reqs])}
    times = {name: [] for name in forms}
    first = {}
    index.profile_enable(False)
    for it in range(args.warmup + args.repeats):
        for name, batch in forms.items():  # alternating
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = veloci_amd.search_batch_flat(batch, index, stride=10)
            ms = (time.perf_counter() - t) * 1e3
            assert not res[4].any(), (name, res[4][res[4] != 0][:4])
            if it == 0:
                first[name] = res
            if it >= args.warmup:
                times[name].append(ms)
    same = all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               for a, b in zip(first["set"][:4], first["filter"][:4]))
    kernels = {}
    for name, batch in forms.items():  # one profiled step each: which kernels ran, and their device time
        index.profile_enable(True)
        index.profile_json(reset=True)
        veloci_amd.search_batch_flat(batch, index, stride=10)
        prof = index.profile_json(reset=True)
        kernels[name] = {kn: {"ms": round(kv["ms"], 3), "launches": kv["launches"], "layout_MB": round(kv["layout_bytes"] / 1e6, 1)}
                         for kn, kv in prof.get("kernels", {}).items() if kv.get("launches")}
        index.profile_enable(False)
    st = {name: stats(v) for name, v in times.items()}
    spread = st["filter"]["max"] - st["filter"]["min"]
    row = {"tree": T, "set_ids": len(ds), "set_device_bytes": ds.device_bytes, "rows_equal": bool(same), "hits_first_queries": first["set"][0][:4].tolist(), "step_ms": st,
           "requests_per_s": {name: round(args.batch / (s["median"] * 1e-3)) for name, s in st.items()}, "filter_form_spread_ms": round(spread, 4),
           "set_not_slower_beyond_the_spread": bool(st["set"]["median"] <= st["filter"]["median"] + spread), "kernels": kernels}
    out["use"].append(row)
    print(json.dumps(row), flush=True)
    assert same, "the set form and the filter form answered differently"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print("DOCSET_FILTER_BENCH_OK", flush=True)


if __name__ == "__main__":
    main()
