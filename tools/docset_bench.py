"""Doc sets on the bench index (profiles/docset/README.md holds the results):

  creation   sets of --sizes ids (random, on the device) on the --docs index: HIP event times of the three stages (VQ_DOCSET_TIMING=1: marking the
             ids, counting + scanning, expanding) and the wall time of vq_docset_create, after a warm-up, --repeats times each
  step       a --batch-request step of 3-term ANDs (the bench's triples) restricted to a 1 % and to a 30 % set, through vq_search_batch_flat: with
             the set as a DocSet, and — the yardstick — with the same ids as the text_id_to_anchor row of a term of an `acl` field and a filter
             leaf on that term.  The two forms alternate, --repeats timed steps each after --warmup; the yardstick's own spread is the noise.
             The first step's rows of the two forms are compared: they must be the same.

usage: python tools/docset_bench.py [--docs 100000000] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("VQ_DOCSET_TIMING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--terms", type=int, default=100_000)
    ap.add_argument("--triples", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sizes", default="10000,1000000,30000000")
    ap.add_argument("--fractions", default="0.01,0.3")
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
    fractions = [float(f) for f in args.fractions.split(",")]
    rows = [np.flatnonzero(rng.random(args.docs) < f).astype(np.uint32) for f in fractions]
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    data.add_fst("acl.textindex", [b"g%d" % k for k in range(len(rows))])
    data.add_key_value_store("acl.textindex.text_id_to_anchor", off, np.concatenate(rows))
    index = veloci_amd.Index(data, device=0)
    out = {"docs": args.docs, "batch": args.batch, "build_s": round(time.time() - t0, 1), "creation": [], "step": []}
    print(f"index: {args.docs} docs, {index.device_bytes / 1e9:.2f} GB, {out['build_s']} s", flush=True)

    # ---- creation
    for n in [int(s) for s in args.sizes.split(",")]:
        n = min(n, args.docs)
        ids = torch.randint(0, args.docs, (n,), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        mark, scan, expand, wall = [], [], [], []
        for it in range(args.warmup + args.repeats):
            t = time.perf_counter()
            ds = veloci_amd.DocSet(index, ids)
            w = (time.perf_counter() - t) * 1e3
            tm = ds.timings()
            uniq, nbytes = len(ds), ds.device_bytes
            ds.close()
            if it >= args.warmup:
                mark.append(tm[0]), scan.append(tm[1]), expand.append(tm[2]), wall.append(w)
        row = {"ids": n, "unique": uniq, "device_bytes": nbytes, "mark_ms": stats(mark), "count_scan_ms": stats(scan), "expand_ms": stats(expand), "create_wall_ms": stats(wall)}
        out["creation"].append(row)
        print(json.dumps(row), flush=True)

    # ---- a step under a set against the same step under the acl filter leaf
    reqs = [synth.req_and(list(meta.triples[i % len(meta.triples)]), top=10) for i in range(args.batch)]
    for k, (f, ids) in enumerate(zip(fractions, rows)):
        ds = veloci_amd.DocSet(index, ids)
        leaf = {"search": {"path": "acl", "terms": ["g%d" % k]}}
        forms = {"docset": veloci_amd.RequestBatch(reqs, docsets=[ds] * len(reqs)), "filter_leaf": veloci_amd.RequestBatch([dict(r, filter=leaf) for r in reqs])}
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
                   for a, b in zip(first["docset"][:4], first["filter_leaf"][:4]))
        kernels = {}
        for name, batch in forms.items():  # one profiled step each: which kernels ran, and their device time
            index.profile_enable(True)
            index.profile_json(reset=True)
            veloci_amd.search_batch_flat(batch, index, stride=10)
            prof = index.profile_json(reset=True)
            kernels[name] = {kn: {"ms": round(kv["ms"], 3), "launches": kv["launches"], "layout_MB": round(kv["layout_bytes"] / 1e6, 1)}
                             for kn, kv in prof.get("kernels", {}).items() if kv.get("launches")}
            index.profile_enable(False)
        row = {"fraction": f, "set_ids": int(len(ids)), "set_device_bytes": ds.device_bytes, "rows_equal": bool(same), "hits_first_queries": first["docset"][0][:4].tolist(),
               "step_ms": {name: stats(v) for name, v in times.items()},
               "requests_per_s": {name: round(args.batch / (stats(v)["median"] * 1e-3)) for name, v in times.items()}, "kernels": kernels}
        out["step"].append(row)
        print(json.dumps(row), flush=True)
        assert same, "the doc-set form and the filter-leaf form answered differently"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print("DOCSET_BENCH_OK", flush=True)


if __name__ == "__main__":
    main()
