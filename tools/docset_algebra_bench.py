"""Doc set algebra on a --docs-anchor index (profiles/docset_algebra/README.md holds the results):

  combine    AND, OR and MINUS of two staged sets of --sizes ids each (random, distinct), every pair of sizes (MINUS in both directions): the wall
             time of vq_docset_combine and the HIP event times of its phases (VQ_DOCSET_TIMING=1: the route's kernels are the "mark" phase, then
             counting + scanning, then expanding), after a warm-up, --repeats times; the route the rule took
  host       the same result the only way there was before, in the same run: ids() downloads both operands, numpy combines them
             (assume_unique: the ids are sorted and unique), DocSet(index, ids) uploads them and builds the image.  The two forms alternate; the result
             lengths must agree, and for results of up to --compare ids the ids themselves
  routes     AND of the smallest with the largest set under both routes (VQ_NO_SETOP_PROBE), alternating

usage: python tools/docset_algebra_bench.py [--docs 100000000] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("VQ_DOCSET_TIMING", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

HOST_OPS = {"and": np.intersect1d, "or": np.union1d, "minus": np.setdiff1d}


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def small_index(veloci_amd, docs):
    """all a doc set needs of its index is the doc range: one two-term field"""
    data = veloci_amd.IndexData(docs)
    offsets = np.array([0, 3, 5], np.uint64)
    anchors = np.array([1, docs // 3, docs - 2, 2, docs // 2], np.uint32)
    data.add_fst("body.textindex", [b"alpha", b"beta"])
    data.add_token_to_anchor_score("body.textindex.to_anchor_id_score", offsets, anchors, np.full(5, 10, np.uint32), None)
    data.add_key_value_store("body.textindex.text_id_to_anchor", offsets, anchors)
    data.set_column_meta("body", False, True)
    return veloci_amd.Index(data, device=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--sizes", default="1000,1000000,40000000")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-repeats", type=int, default=2, help="timed host round trips per row (the large ones take seconds each)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--compare", type=int, default=2_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import veloci_amd
    if not torch.cuda.is_available():
        raise SystemExit("docset_algebra_bench: no GPU (a timing taken anywhere else says nothing)")

    t0 = time.time()
    index = small_index(veloci_amd, args.docs)
    sizes = [min(int(s), args.docs) for s in args.sizes.split(",")]
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    sets = {}
    for side in ("a", "b"):  # two independent sets per size
        perm = torch.randperm(args.docs, device="cuda:0", generator=gen)
        for n in sizes:
            ids = perm[:n].to(torch.int32).contiguous()
            torch.cuda.synchronize()
            sets[(side, n)] = veloci_amd.DocSet(index, ids)
        del perm
    out = {"docs": args.docs, "sizes": sizes, "build_s": round(time.time() - t0, 1), "operands": [], "combine": [], "routes": []}
    for (side, n), ds in sets.items():
        out["operands"].append({"set": side + str(n), "ids": len(ds), "bitmap": int(veloci_amd.lib().vq_debug_docset_part(ds._handle(), 1, None, 0)) > 0, "device_bytes": ds.device_bytes})
    print(json.dumps(out["operands"]), flush=True)

    def device_form(op, x, y):
        t = time.perf_counter()
        ds = veloci_amd.DocSet.combine(index, op, [x, y])
        return ds, (time.perf_counter() - t) * 1e3

    def host_form(op, x, y):
        t = time.perf_counter()
        ids = HOST_OPS[op](x.ids(), y.ids(), assume_unique=True) if op != "or" else np.union1d(x.ids(), y.ids())
        ds = veloci_amd.DocSet(index, ids)
        return ds, (time.perf_counter() - t) * 1e3

    # ---- every pair of sizes, device against the host round trip
    pairs = [(na, nb) for i, na in enumerate(sizes) for nb in sizes[i:]]
    for op in ("and", "or", "minus"):
        for na, nb in pairs + ([(nb, na) for na, nb in pairs if na != nb] if op == "minus" else []):
            x, y = sets[("a", na)], sets[("b", nb)]
            wall, mark, scan, expand, host = [], [], [], [], []
            for it in range(args.warmup + args.repeats):
                ds, ms = device_form(op, x, y)
                tm, route, n_out = ds.timings(), ds.route, len(ds)
                if it >= args.warmup:
                    wall.append(ms), mark.append(tm[0]), scan.append(tm[1]), expand.append(tm[2])
                if args.warmup <= it < args.warmup + args.host_repeats or it == 0:  # alternating with the device form (the first one is the warm-up)
                    hs, hms = host_form(op, x, y)
                    assert len(hs) == n_out, (op, na, nb, len(hs), n_out)
                    if n_out <= args.compare:
                        assert np.array_equal(hs.ids(), ds.ids()), (op, na, nb)
                    hs.close()
                    if it >= args.warmup:
                        host.append(hms)
                ds.close()
            row = {"op": op, "a": na, "b": nb, "result_ids": n_out, "route": route, "combine_wall_ms": stats(wall), "mark_ms": stats(mark), "count_scan_ms": stats(scan),
                   "expand_ms": stats(expand), "host_round_trip_ms": stats(host), "speedup": round(stats(host)["median"] / stats(wall)["median"], 1)}
            out["combine"].append(row)
            print(json.dumps(row), flush=True)

    # ---- both routes on one input: the smallest set and-ed with the largest
    x, y = sets[("a", sizes[0])], sets[("b", sizes[-1])]
    times = {"probe": {"wall": [], "mark": []}, "words": {"wall": [], "mark": []}}
    for it in range(args.warmup + args.repeats):
        for name in times:  # alternating
            if name == "words":
                os.environ["VQ_NO_SETOP_PROBE"] = "1"
            try:
                ds, ms = device_form("and", x, y)
            finally:
                os.environ.pop("VQ_NO_SETOP_PROBE", None)
            assert ds.route == (0 if name == "words" else 1), (name, ds.route)
            if it >= args.warmup:
                times[name]["wall"].append(ms), times[name]["mark"].append(ds.timings()[0])
            n_out = len(ds)
            ds.close()
    row = {"op": "and", "a": sizes[0], "b": sizes[-1], "result_ids": n_out, "probe": {k: stats(v) for k, v in times["probe"].items()},
           "words": {k: stats(v) for k, v in times["words"].items()}}
    out["routes"].append(row)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print("DOCSET_ALGEBRA_BENCH_OK", flush=True)


if __name__ == "__main__":
    main()
