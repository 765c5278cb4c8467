"""A doc set ordered by a column on the bench index (profiles/docset_top/README.md holds the results).

On the --docs index with its `pop` column (f32 in [1, 1e5), every doc present) and a derived column `grade` of 10 distinct values (the tie-heavy
case), for sets of --sets random ids and pages of --tops rows:

  yardstick   what a caller has without the entry point (--yardstick-only runs nothing else and needs nothing of it, so it also runs on an older
              build of the library: VQ_BENCH_TREE=<that checkout>): ds.ids() to the host, a host copy of the column, np.argpartition for the page
              and a sort of the page by (value, doc)
  new path    ds.top_by(field, top=): wall time of the call and the HIP event time of its kernels (VQ_DOCSET_TIMING=1, vq_debug_docset_top_ms);
              the rows are held against numpy's full lexsort at every size
  reported    torch.topk over column_tensor[ds.ids_tensor()] (a caller who keeps a second copy of the column as a torch tensor; values only, its
              tie order is not the doc id's); the bytes the kernels move over the kernel time; the final order of a page of K pairs made on the host after the download against a
              device radix sort before it

--repeats timed calls each after --warmup; medians with min and max.

usage: python tools/docset_top_bench.py [--docs 100000000] [--yardstick-only] [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("VQ_DOCSET_TIMING", "1")
# VQ_BENCH_TREE: the checkout whose veloci_amd package (and library) is measured — the parent commit's for the yardstick; default: this one
sys.path.insert(0, os.environ.get("VQ_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

LINE = 128  # bytes of a cache line: what one gathered value costs at least


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=100_000_000)
    ap.add_argument("--terms", type=int, default=100_000)
    ap.add_argument("--sets", default="200,1000000,40000000")
    ap.add_argument("--tops", default="10,1000,65536")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
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
    grade = np.floor(np.log10(pop) * 2.0).astype(np.float32)  # 10 distinct values (0 .. 9): every key has millions of ties
    columns = {"pop": pop, "grade": grade}
    data.add_boost("grade.boost_valid_to_value", grade, None, key_base=0)
    index = veloci_amd.Index(data, device=0)
    out = {"docs": args.docs, "lib": os.path.basename(veloci_amd._lib.lib_path()), "build_s": round(time.time() - t0, 1), "grade_values": int(np.unique(grade).size), "sets": []}
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
                    kern.append(float(L.vq_debug_docset_top_ms()))
        return wall, kern, first

    rng = np.random.default_rng(9)
    tops = [int(t) for t in args.tops.split(",")]
    for size in [int(s) for s in args.sets.split(",")]:
        size = min(size, args.docs)
        ids = np.flatnonzero(rng.random(args.docs) < size / args.docs) if size * 20 > args.docs else np.sort(rng.choice(args.docs, size=size, replace=False))
        ds = veloci_amd.DocSet(index, ids)
        row = {"set_ids": int(ids.size), "set_has_bitmap": bool(ds.part(1).size), "pages": []}
        for field, col in columns.items():
            order = np.lexsort((ids, col[ids])) if not args.yardstick_only else None  # the check: the whole set in the order
            col_t = torch.from_numpy(col).to("cuda:0") if not args.yardstick_only else None
            for top in tops:
                k = min(top, int(ids.size))

                def by_numpy():
                    mine = ds.ids()
                    v = col[mine]
                    if 0 < k < mine.size:
                        # the k smallest by value; ties at the cut go by doc id: everything below the k-th value, then the first ids equal to it
                        kth = v[np.argpartition(v, k - 1)[:k]].max()
                        less = np.flatnonzero(v < kth)
                        cand = np.concatenate([less, np.flatnonzero(v == kth)[:k - less.size]])
                    else:
                        cand = np.arange(mine.size)
                    page = cand[np.lexsort((mine[cand], v[cand]))][:k]
                    return mine[page], v[page]

                wall, _, y = timed(by_numpy)
                page = {"field": field, "top": top, "yardstick_ids_numpy_partition_sort_wall_ms": stats(wall)}
                if not args.yardstick_only:
                    want_docs, want_vals = ids[order[:k]], col[ids][order[:k]]
                    assert np.array_equal(y[0], want_docs)
                    wall, kern, got = timed(lambda: ds.top_by(field, top=top), True)
                    assert np.array_equal(got.docs, want_docs.astype(np.uint32)) and np.array_equal(got.values.view(np.uint32), want_vals.view(np.uint32)) and not got.kinds.any()
                    assert got.counters == {"docs": int(ids.size), "count": int(ids.size), "nan": 0, "missing": 0}
                    lines = int(np.unique(ids >> 5).size)
                    select = ids.size > top
                    moved = int(ids.size) * 4 + lines * LINE + int(ids.size) * 4 + (int(ids.size) * 4 * 5 + int(ids.size) * 4 if select else int(ids.size) * 8)
                    ms = stats(kern)["median"]
                    page["top_by"] = {"wall_ms": stats(wall), "kernel_ms": stats(kern), "bytes_moved": moved, "achieved_GBps": round(moved / (ms * 1e-3) / 1e9, 1) if ms > 0 else None,
                                      "rows_checked": int(k)}
                    page["speedup_over_yardstick_wall"] = round(page["yardstick_ids_numpy_partition_sort_wall_ms"]["median"] / page["top_by"]["wall_ms"]["median"], 2)
                    wall, _, _ = timed(lambda: ds.top_by(field, top=top, descending=True), True)
                    page["top_by_descending_wall_ms"] = stats(wall)

                    def by_torch():
                        v = col_t[ds.ids_tensor().long()]
                        r = torch.topk(v, k, largest=False, sorted=True)
                        torch.cuda.synchronize()
                        return r.values

                    wall, _, tv = timed(by_torch)
                    assert np.array_equal(tv.cpu().numpy(), want_vals)
                    page["torch_topk_values_only_wall_ms"] = stats(wall)
                    pairs = (np.uint64(1) << np.uint64(32)) * rng.integers(0, 1 << 32, size=k, dtype=np.uint64) + rng.integers(0, 1 << 32, size=k, dtype=np.uint64)
                    # the final order of the page: the pairs downloaded and sorted on the host (what docset_top.cpp does) against a device radix sort
                    # (torch.sort of int64: rocPRIM, as seg_sort_u64 is) followed by the download
                    pairs_t = torch.from_numpy(pairs.view(np.int64) >> 1).to("cuda:0")
                    wall, _, _ = timed(lambda: np.sort(pairs_t.cpu().numpy()))
                    page["final_order_download_then_host_sort_wall_ms"] = stats(wall)
                    wall, _, _ = timed(lambda: torch.sort(pairs_t).values.cpu().numpy())
                    page["final_order_device_sort_then_download_wall_ms"] = stats(wall)
                row["pages"].append(page)
                print(json.dumps(page), flush=True)
            del col_t
        ds.close()
        out["sets"].append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
    print("DOCSET_TOP_BENCH_OK", flush=True)


if __name__ == "__main__":
    main()
