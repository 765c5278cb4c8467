"""Numeric aggregations of a doc set on the bench index (profiles/docset_aggs/README.md holds the results).

On the --docs index with its `pop` column (f32 in [1, 1e5), every doc present), for sets of --sets random ids:

  yardstick   what a caller has without the entry point (--yardstick-only runs nothing else and needs nothing of it, so it also runs on an older
              build of the library: VQ_BENCH_TREE=<that checkout>):
                stats       numpy over a host copy of the column and the set's ids: count, min, max and a float64 sum (not the exact one)
                histogram   16 edges, 17 buckets: 17 calls of DocSet.from_range(index, "pop", gte=, lt=) & ds, each with len(); and, as the stronger
                            form, the same with within=ds, which probes the set's ids when it carries no bitmap
  new path    ds.stats("pop") and ds.histogram("pop", edges): wall time of the call and the HIP event time of the kernels
              (VQ_DOCSET_TIMING=1, vq_debug_docset_aggregate_ms), with the wave pre-reduction of the sum and without it (VQ_NO_AGG_PREREDUCE=1);
              the buckets are held against the 17 calls' lengths, count / min / max against numpy, the sum against math.fsum (sets up to --fsum-max ids)
  1:n         the same two calls on `v[].x`: a column of --docs values, value id v belonging to anchor (v * 48271 + 11) mod docs
  bandwidth   the bytes a kernel must read — ids route: the ids plus every 128-byte line of the column that holds one of their values; values
              route: the column, and beside it the value_id_to_anchor offsets and entries — over the kernel time

--repeats timed calls each after --warmup; medians with min and max.

usage: python tools/docset_aggs_bench.py [--docs 100000000] [--yardstick-only] [--out FILE.json]"""
import argparse
import json
import math
import os
import sys
import time

os.environ.setdefault("VQ_DOCSET_TIMING", "1")
# VQ_BENCH_TREE: the checkout whose veloci_amd package (and library) is measured — the parent commit's for the yardstick; default: this one
sys.path.insert(0, os.environ.get("VQ_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

PEAK_GBPS = 8000.0  # MI355X HBM3E, the specified peak
LINE = 128          # bytes of a cache line: what one gathered value costs at least
EDGES = [float(np.float32(1.0 + (k + 1) * (1e5 - 1.0) / 17.0)) for k in range(16)]  # 17 buckets of about equal share; float32 values: numpy's f32 comparison is the f64 one


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--terms", type=int, default=100_000)
    ap.add_argument("--sets", default="200,1000000,40000000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fsum-max", type=int, default=1_000_000)
    ap.add_argument("--yardstick-only", action="store_true")
    ap.add_argument("--no-1n", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import veloci_amd
    from veloci_amd import synth

    t0 = time.time()
    data, meta = synth.generate(synth.SynthSpec(num_docs=args.docs, num_terms=args.terms, triples=4, with_t2t=False, with_facets=False, with_boost=True, with_phrase=False),
                                device="cuda:0")
    kb, present, bits = data.boost["pop.boost_valid_to_value"]
    assert kb == 0 and present is None and len(bits) == args.docs
    pop = bits.view(np.float32)  # the host copy of the column: what the yardstick's caller has to keep
    with_1n = not args.yardstick_only and not args.no_1n
    if with_1n:
        owner = ((np.arange(args.docs, dtype=np.uint64) * np.uint64(48271) + np.uint64(11)) % np.uint64(args.docs)).astype(np.uint32)
        x_vals = np.roll(pop, 1_000_003)
        data.add_boost("v[].x.boost_valid_to_value", x_vals, None, key_base=0)
        data.add_key_value_store("v[].x.value_id_to_anchor", np.arange(args.docs + 1, dtype=np.uint64), owner)
    index = veloci_amd.Index(data, device=0)
    out = {"docs": args.docs, "lib": os.path.basename(veloci_amd._lib.lib_path()), "build_s": round(time.time() - t0, 1), "peak_GBps_assumed": PEAK_GBPS, "edges": EDGES, "sets": []}
    print(f"index: {args.docs} docs, {index.device_bytes / 1e9:.2f} GB, {out['build_s']} s, {out['lib']}", flush=True)
    rounds = args.warmup + args.repeats
    L = veloci_amd.lib()

    def timed(call, kernel_ms=False):
        """-> (wall ms of the timed calls, kernel ms of the timed calls, the first call's result)"""
        wall, kern, first = [], [], None
        for it in range(rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = call()
            ms = (time.perf_counter() - t) * 1e3
            if it == 0:
                first = got
            if it >= args.warmup:
                wall.append(ms)
                if kernel_ms:
                    kern.append(float(L.vq_debug_docset_aggregate_ms()))
        return wall, kern, first

    rng = np.random.default_rng(9)
    for size in [int(s) for s in args.sets.split(",")]:
        size = min(size, args.docs)
        ids = np.flatnonzero(rng.random(args.docs) < size / args.docs) if size * 20 > args.docs else np.sort(rng.choice(args.docs, size=size, replace=False))
        ds = veloci_amd.DocSet(index, ids)
        row = {"set_ids": int(ids.size), "set_has_bitmap": bool(ds.part(1).size)}

        def np_stats():
            v = pop[ids]
            return int(v.size), float(v.min()), float(v.max()), float(v.sum(dtype=np.float64))

        def by_sets(within):
            counts = []
            for i in range(len(EDGES) + 1):
                b = {}
                if i > 0:
                    b["gte"] = EDGES[i - 1]
                if i < len(EDGES):
                    b["lt"] = EDGES[i]
                if within:
                    r = veloci_amd.DocSet.from_range(index, "pop", within=ds, **b)
                    counts.append(len(r))
                else:
                    r = veloci_amd.DocSet.from_range(index, "pop", **b)
                    c = r & ds
                    counts.append(len(c))
                    c.close()
                r.close()
            return counts

        wall, _, y_stats = timed(np_stats)
        row["yardstick_numpy_stats_wall_ms"] = stats(wall)
        wall, _, y_hist = timed(lambda: by_sets(False))
        row["yardstick_17_from_range_and_ds_wall_ms"] = stats(wall)
        wall, _, y_hist_w = timed(lambda: by_sets(True))
        row["yardstick_17_from_range_within_ds_wall_ms"] = stats(wall)
        assert y_hist == y_hist_w and sum(y_hist) == ids.size, (y_hist, y_hist_w)
        row["buckets"] = y_hist
        if not args.yardstick_only:
            lines = int(np.unique(ids >> 5).size)
            must_read = int(ids.size) * 4 + lines * LINE
            row["ids_route_bytes_must_read"] = must_read
            for mode, env in (("prereduce", None), ("no_prereduce", "1")):
                if env:
                    os.environ["VQ_NO_AGG_PREREDUCE"] = env
                try:
                    wall, kern, st = timed(lambda: ds.stats("pop"), True)
                    assert (st["count"], st["min"], st["max"]) == y_stats[:3] and st["missing"] == 0 and st["nan"] == 0, (st, y_stats)
                    if ids.size <= args.fsum_max:
                        assert st["sum"] == math.fsum(pop[ids].astype(np.float64).tolist()), st
                        row["sum_equals_fsum"] = True
                    row["sum_minus_numpy_float64_sum"] = st["sum"] - y_stats[3]
                    ms = stats(kern)["median"]
                    row["stats_%s" % mode] = {"wall_ms": stats(wall), "kernel_ms": stats(kern), "achieved_GBps": round(must_read / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
                    wall, kern, hist = timed(lambda: ds.histogram("pop", EDGES), True)
                    assert hist == y_hist, (hist, y_hist)
                    ms = stats(kern)["median"]
                    row["histogram_%s" % mode] = {"wall_ms": stats(wall), "kernel_ms": stats(kern), "achieved_GBps": round(must_read / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
                finally:
                    os.environ.pop("VQ_NO_AGG_PREREDUCE", None)
            row["histogram_speedup_over_17_calls"] = round(row["yardstick_17_from_range_and_ds_wall_ms"]["median"] / row["histogram_prereduce"]["wall_ms"]["median"], 1)
            row["histogram_speedup_over_17_calls_within"] = round(row["yardstick_17_from_range_within_ds_wall_ms"]["median"] / row["histogram_prereduce"]["wall_ms"]["median"], 1)
            if with_1n:
                member = np.zeros(args.docs, bool)
                member[ids] = True
                sel = member[owner]
                want_count = int(sel.sum())
                col_bytes, table_bytes = args.docs * 4, args.docs * 12
                for mode, env in (("prereduce", None), ("no_prereduce", "1")):
                    if env:
                        os.environ["VQ_NO_AGG_PREREDUCE"] = env
                    try:
                        wall, kern, st = timed(lambda: ds.stats("v[].x"), True)
                        assert st["count"] == want_count and st["missing"] == 0 and st["max"] == float(x_vals[sel].max()), (st, want_count)
                        ms = stats(kern)["median"]
                        row["one_to_n_stats_%s" % mode] = {"wall_ms": stats(wall), "kernel_ms": stats(kern), "values_aggregated": want_count,
                                                          "column_GBps": round(col_bytes / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                                                          "column_and_table_GBps": round((col_bytes + table_bytes) / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
                        wall, kern, hist = timed(lambda: ds.histogram("v[].x", EDGES), True)
                        assert sum(hist) == want_count
                        row["one_to_n_histogram_%s" % mode] = {"wall_ms": stats(wall), "kernel_ms": stats(kern)}
                    finally:
                        os.environ.pop("VQ_NO_AGG_PREREDUCE", None)
                del member, sel
        ds.close()
        out["sets"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print("DOCSET_AGGS_BENCH_OK", flush=True)


if __name__ == "__main__":
    main()
