"""Facet counts of a doc set on the bench index (profiles/docset_facets/README.md holds the results):

  new route   ds.facets([{"field": "cat"}, {"field": "tags[]", "top": 10}]) for sets of --sizes ids on the --docs index, in both counting modes
              (VQ_NO_DOCSET_FACET_LDS flipped between calls): the wall time of the call and the HIP event time of the count kernel
              (VQ_DOCSET_TIMING=1, vq_debug_docset_facets_count_ms), --repeats timed calls each after --warmup, the spread reported
  yardstick   the only route to the same answer without vq_docset_facets: every set indexed as the row of a term of an `acl` field and a scored
              search {search_req: the acl leaf, top: 1, facets: the same}.  --yardstick-only runs nothing else and needs nothing of the new entry
              point, so it also runs on an older build of the library (VQ_LIB=<that build>) on the same box
  The two routes' facets are compared on the first call: they must be the same.

usage: python tools/docset_facets_bench.py [--docs 100000000] [--yardstick-only] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("VQ_DOCSET_TIMING", "1")
# VQ_BENCH_TREE: the checkout whose veloci_amd package (and library) is measured — the parent commit's for the yardstick; default: this one
sys.path.insert(0, os.environ.get("VQ_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

FACETS = [{"field": "cat"}, {"field": "tags[]", "top": 10}]


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--terms", type=int, default=100_000)
    ap.add_argument("--sizes", default="300,1000000,40000000")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import veloci_amd
    from veloci_amd import synth

    t0 = time.time()
    data, meta = synth.generate(synth.SynthSpec(num_docs=args.docs, num_terms=args.terms, triples=4, with_t2t=False, with_facets=True, with_boost=False, with_phrase=False),
                                device="cuda:0")
    rng = np.random.default_rng(3)
    sizes = [min(int(s), args.docs) for s in args.sizes.split(",")]
    rows = [np.flatnonzero(rng.random(args.docs) < n / args.docs).astype(np.uint32) if n > 100_000 else np.sort(rng.choice(args.docs, size=n, replace=False)).astype(np.uint32)
            for n in sizes]
    off = np.zeros(len(rows) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    vals = np.concatenate(rows)
    data.add_fst("acl.textindex", [b"g%d" % k for k in range(len(rows))])
    data.add_token_to_anchor_score("acl.textindex.to_anchor_id_score", off, vals, np.full(len(vals), 10, np.uint32), None)
    data.add_key_value_store("acl.textindex.text_id_to_anchor", off, vals)
    index = veloci_amd.Index(data, device=0)
    L = veloci_amd.lib()
    out = {"docs": args.docs, "lib": os.path.basename(veloci_amd._lib.lib_path()), "facets": FACETS, "build_s": round(time.time() - t0, 1), "rows": []}
    print(f"index: {args.docs} docs, {index.device_bytes / 1e9:.2f} GB, {out['build_s']} s, {out['lib']}", flush=True)
    # bytes the kernel's layout must move per id: the id, cat's direct value, tags[]'s two offsets and its values
    kb, toff, _ = data.key_value_stores["tags[].textindex.anchor_to_text_id"]
    for k, ids in enumerate(rows):
        row = {"set_ids": int(len(ids))}
        req = veloci_amd.Request({"search_req": {"search": {"path": "acl", "terms": ["g%d" % k]}}, "top": 1, "facets": FACETS})
        wall, first = [], {}
        for it in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = veloci_amd.search(req, index)
            ms = (time.perf_counter() - t) * 1e3
            if it == 0:
                first["yardstick"] = res
            if it >= args.warmup:
                wall.append(ms)
        assert first["yardstick"].num_hits == len(ids)
        row["yardstick_search_top1_wall_ms"] = stats(wall)
        if not args.yardstick_only:
            ds = veloci_amd.DocSet(index, ids)
            n_tag_values = int(toff[ids.astype(np.int64) - kb + 1].astype(np.int64).sum() - toff[ids.astype(np.int64) - kb].astype(np.int64).sum())
            row["layout_bytes"] = {"cat": int(len(ids)) * (4 + 4), "tags[]": int(len(ids)) * (4 + 16) + 4 * n_tag_values}
            for mode in ("lds", "cache"):
                if mode == "cache":
                    os.environ["VQ_NO_DOCSET_FACET_LDS"] = "1"
                wall, kern = [], []
                for it in range(args.warmup + args.repeats):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    res = ds.facet_result(FACETS)
                    ms = (time.perf_counter() - t) * 1e3
                    if it == 0:
                        first[mode] = res
                    if it >= args.warmup:
                        wall.append(ms)
                        kern.append(float(L.vq_debug_docset_facets_count_ms()))
                os.environ.pop("VQ_NO_DOCSET_FACET_LDS", None)
                assert first[mode].num_hits == len(ids) and first[mode].facets == first["yardstick"].facets, mode
                row[mode] = {"call_wall_ms": stats(wall), "count_kernel_ms": stats(kern)}
                total = sum(row["layout_bytes"].values())
                row[mode]["count_kernel_GBps_of_layout_bytes"] = round(total / (stats(kern)["median"] * 1e-3) / 1e9, 1) if stats(kern)["median"] > 0 else None
            row["facets_equal_yardstick"] = True
            ds.close()
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print("DOCSET_FACETS_BENCH_OK", flush=True)


if __name__ == "__main__":
    main()
