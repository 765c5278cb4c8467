"""Doc sets from numeric ranges on the bench index (profiles/docset_ranges/README.md holds the results):

  stream route   DocSet.from_ranges over the `pop` column (f32 in [1, 1e5), every doc present) of the --docs index with one clause and with four
                 clauses (pop and three rotated copies of it, p1 .. p3, so that every clause streams a column of its own): the HIP event time of
                 marking (VQ_DOCSET_TIMING=1, vq_debug_docset_timings: k_range_bits alone) and the fraction it achieves of the bytes the route
                 must move — 4 B per doc and clause, plus 1 bit per doc written — at --selectivities of the docs selected
  probe route    the same one-clause and four-clause sets under a `within` of 200 and of 1 M random ids (no bitmap): marking is k_range_probe
  whole call     DocSet.from_range(index, "pop", gte, lt) as Python sees it against the only route to the same set without the entry point: the
                 column held on the host, numpy's mask, DocSet(index, np.flatnonzero(mask)).  --yardstick-only runs nothing else and needs nothing
                 of the new entry point, so it also runs on an older build of the library (VQ_BENCH_TREE=<that checkout>) on the same box
  The two routes' ids are compared on the first call: they must be the same.

--repeats timed calls each after --warmup; medians with min and max.

usage: python tools/docset_ranges_bench.py [--docs 100000000] [--yardstick-only] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("VQ_DOCSET_TIMING", "1")
# VQ_BENCH_TREE: the checkout whose veloci_amd package (and library) is measured — the parent commit's for the yardstick; default: this one
sys.path.insert(0, os.environ.get("VQ_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

PEAK_GBPS = 8000.0  # MI355X HBM3E, the specified peak: the fractions below are against it (a plain float4 copy reaches about 6300)


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--terms", type=int, default=100_000)
    ap.add_argument("--selectivities", default="0.001,0.1,0.5")
    ap.add_argument("--withins", default="200,1000000")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yardstick-only", action="store_true")
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
    cols = ["pop", "p1", "p2", "p3"]
    for k in (1, 2, 3):
        data.add_boost("p%d.boost_valid_to_value" % k, np.roll(pop, 1_000_003 * k), None, key_base=0)
    index = veloci_amd.Index(data, device=0)
    out = {"docs": args.docs, "lib": os.path.basename(veloci_amd._lib.lib_path()), "build_s": round(time.time() - t0, 1), "peak_GBps_assumed": PEAK_GBPS, "whole_call": []}
    print(f"index: {args.docs} docs, {index.device_bytes / 1e9:.2f} GB, {out['build_s']} s, {out['lib']}", flush=True)
    rounds = args.warmup + args.repeats

    def timed(make):
        """-> (wall ms of the timed calls, mark ms of the timed calls, the first call's ids, its length)"""
        wall, mark, first = [], [], None
        for it in range(rounds):
            torch.cuda.synchronize()
            t = time.perf_counter()
            ds = make()
            ms = (time.perf_counter() - t) * 1e3
            if it == 0:
                first = (ds.ids(), len(ds))
            if it >= args.warmup:
                wall.append(ms)
                tm = ds.timings()
                mark.append(tm[0] if tm else -1.0)
            ds.close()
        return wall, mark, first[0], first[1]

    def interval(sel):
        lo = 1000.0  # pop is uniform in [1, 1e5); both bounds are float32 values, so numpy's float32 comparison is the float64 one
        return lo, float(np.float32(lo + sel * (1e5 - 1.0)))

    for sel in [float(s) for s in args.selectivities.split(",")]:
        lo, hi = interval(sel)
        row = {"selectivity": sel, "gte": lo, "lt": hi}

        def yardstick():
            mask = (pop >= np.float32(lo)) & (pop < np.float32(hi))
            return veloci_amd.DocSet(index, np.flatnonzero(mask))
        assert float(np.float32(lo)) == lo and float(np.float32(hi)) == hi, (lo, hi)
        wall, _, y_ids, y_len = timed(yardstick)
        row["set_ids"] = int(y_len)
        row["yardstick_numpy_then_DocSet_wall_ms"] = stats(wall)
        t = time.perf_counter()
        mask = (pop >= np.float32(lo)) & (pop < np.float32(hi))
        ids = np.flatnonzero(mask)
        row["yardstick_numpy_part_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        del mask, ids
        if not args.yardstick_only:
            wall, mark, ids, n = timed(lambda: veloci_amd.DocSet.from_range(index, "pop", gte=lo, lt=hi))
            assert n == y_len and np.array_equal(ids, y_ids), sel
            row["from_range_wall_ms"], row["from_range_mark_ms"], row["ids_equal_yardstick"] = stats(wall), stats(mark), True
        out["whole_call"].append(row)
        print(json.dumps(row), flush=True)

    if not args.yardstick_only:
        out["stream"], out["probe"] = [], []
        for sel in [float(s) for s in args.selectivities.split(",")]:
            lo, hi = interval(sel)
            for n_clauses in (1, 4):
                # four clauses: each column's interval is wider, so that the conjunction still selects about `sel` of the docs
                width = (sel ** (1.0 / n_clauses)) * (1e5 - 1.0)
                clauses = [{"field": cols[k], "gte": 1000.0, "lt": 1000.0 + width} for k in range(n_clauses)]
                wall, mark, ids, n = timed(lambda: veloci_amd.DocSet.from_ranges(index, clauses))
                must_move = args.docs * 4 * n_clauses + args.docs // 8
                ms = stats(mark)["median"]
                row = {"clauses": n_clauses, "target_selectivity": sel, "set_ids": int(n), "mark_ms": stats(mark), "call_wall_ms": stats(wall), "bytes_must_move": must_move,
                       "achieved_GBps": round(must_move / (ms * 1e-3) / 1e9, 1) if ms > 0 else None}
                row["fraction_of_peak"] = round(row["achieved_GBps"] / PEAK_GBPS, 3) if row["achieved_GBps"] else None
                out["stream"].append(row)
                print(json.dumps(row), flush=True)
        rng = np.random.default_rng(9)
        for size in [int(s) for s in args.withins.split(",")]:
            w_ids = np.sort(rng.choice(args.docs, size=min(size, args.docs), replace=False))
            within = veloci_amd.DocSet(index, w_ids)
            assert within.part(1).size == 0, "the within set carries a bitmap: the probe route would not be taken"
            for n_clauses in (1, 4):
                clauses = [{"field": cols[k], "gte": 1000.0, "lt": 60000.0} for k in range(n_clauses)]
                wall, mark, ids, n = timed(lambda: veloci_amd.DocSet.from_ranges(index, clauses, within=within))
                ds = veloci_amd.DocSet.from_ranges(index, clauses, within=within)
                assert ds.range_route == 1
                ds.close()
                os.environ["VQ_NO_RANGE_PROBE"] = "1"
                try:
                    s_wall, s_mark, s_ids, s_n = timed(lambda: veloci_amd.DocSet.from_ranges(index, clauses, within=within))
                finally:
                    del os.environ["VQ_NO_RANGE_PROBE"]
                assert np.array_equal(ids, s_ids) and n == s_n
                want = np.ones(w_ids.size, bool)
                for k in range(n_clauses):
                    v = np.roll(pop, 1_000_003 * k)[w_ids] if k else pop[w_ids]
                    want &= (v >= np.float32(1000.0)) & (v < np.float32(60000.0))
                assert np.array_equal(ids, w_ids[want].astype(np.uint32))
                row = {"within_ids": int(w_ids.size), "clauses": n_clauses, "set_ids": int(n), "probe_mark_ms": stats(mark), "probe_call_wall_ms": stats(wall),
                       "stream_route_mark_ms": stats(s_mark), "stream_route_call_wall_ms": stats(s_wall), "ids_equal_numpy": True}
                out["probe"].append(row)
                print(json.dumps(row), flush=True)
            within.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print("DOCSET_RANGES_BENCH_OK", flush=True)


if __name__ == "__main__":
    main()
