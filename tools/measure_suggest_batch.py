"""Batched suggest against a loop of single suggests (needs a GPU).

    python tools/measure_suggest_batch.py --parent-tree <checkout of the parent commit, library built> [--out DIR, default profiles/suggest_batch/run] [--terms 300000,1000000]

256 requests of the reference generator's shape (query_generator.rs:288-322: one part per field, starts_with, top 10 on every part) over
widecorpus dictionaries (8 lowercase letters per term, first letter one of four): prefixes of 1, 2, 3 and 5 letters in equal parts, one part
and three parts (three fields with the same terms).  Two legs, each in child processes of their own under `timeout`:
  single   a loop of 256 vq_suggest_json calls on the PARENT commit (--parent-tree: its Python package and its library): the baseline
  batch    one vq_suggest_batch call on this tree's library
Per leg: the median, minimum and maximum wall time of >= 20 repetitions after 5 warm-ups (a call ends in a device synchronisation).  For the
batch also the device time per call of k_dict_scan, the grouping step and k_dict_topn from vq_profile_json (the parent's single path does not
account its launches there), and the bytes copied back: for the batch 8 per entry of a top-n buffer (vq_index_suggest_topn_probes) plus its
segment / offset / count tables, every probe being a top-n probe (asserted; a full-route record would be 12 bytes); 12 per match for the single
path (matches counted from the dictionary).  The answers of both legs are compared.  Writes suggest_batch.json and a
markdown table into --out; after a child that fails or runs into its time limit nothing more is started."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ("body", "title", "alias")
N_REQUESTS = 256


def build(num_terms):
    import numpy as np
    import widecorpus
    data, terms = widecorpus.build(num_terms=num_terms, num_docs=1_000_000, planted=False)
    offsets = np.arange(len(terms) + 1, dtype=np.uint64)
    anchors = (np.arange(len(terms)) % 1_000_000).astype(np.uint32)
    for f in FIELDS[1:]:  # the same dictionary under two more fields, one posting per term
        data.add_fst(f + ".textindex", terms)
        data.add_token_to_anchor_score(f + ".textindex.to_anchor_id_score", offsets, anchors, np.full(len(terms), 10, np.uint32), None)
        data.add_key_value_store(f + ".textindex.text_id_to_anchor", offsets, anchors)
    return data, terms


def requests(terms, parts):
    import numpy as np
    rng = np.random.default_rng(2024)
    out, prefixes = [], []
    for k, n_letters in enumerate((1, 2, 3, 5)):
        for t in rng.integers(0, len(terms), size=N_REQUESTS // 4):
            prefix = terms[int(t)].decode()[:n_letters]
            prefixes.append(prefix)
            ps = [{"path": f, "terms": [prefix], "starts_with": True, "levenshtein_distance": 0, "top": 10, "skip": 0} for f in FIELDS[:parts]]
            out.append(json.dumps({"suggest": ps, "top": 10, "skip": 0}))
    return out, prefixes


def child(args):
    if args.tree:  # the parent commit's package and library instead of this tree's
        sys.path.insert(0, os.path.abspath(args.tree))
    import veloci_amd
    from veloci_amd import _lib
    data, terms = build(args.child_terms)
    idx = veloci_amd.Index(data, device=0)
    assert os.path.abspath(_lib.lib_path()).startswith(os.path.abspath(args.tree or ROOT)), _lib.lib_path()
    result = {"leg": args.leg, "terms": len(terms), "lib": os.path.relpath(_lib.lib_path(), os.path.abspath(args.tree or ROOT)), "parts": {}}
    for parts in (1, 3):
        reqs, prefixes = requests(terms, parts)
        by_len = {}
        import bisect
        for p in set(prefixes):
            lo, hi = bisect.bisect_left(terms, p.encode()), bisect.bisect_left(terms, p.encode() + b"\xff")
            by_len[p] = hi - lo
        matches = sum(by_len[p] for p in prefixes) * parts
        if args.leg == "single":
            run = lambda: [veloci_amd.suggest(r, idx) for r in reqs]  # noqa: E731
        else:
            run = lambda: veloci_amd.suggest_batch(reqs, idx)  # noqa: E731
        for _ in range(args.warmup):
            answers = run()
        row = {"matches_per_call": matches}
        if args.leg == "batch":
            a0, b0 = C.c_uint64(), C.c_uint64()
            _lib.lib().vq_index_suggest_topn_probes(idx.h, C.byref(a0), C.byref(b0))
        times = []
        for _ in range(args.reps):
            t = time.perf_counter()
            answers = run()
            times.append((time.perf_counter() - t) * 1e3)
        row.update(median_ms=round(statistics.median(times), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3), reps=len(times))
        if args.leg == "batch":
            a1, b1 = C.c_uint64(), C.c_uint64()
            _lib.lib().vq_index_suggest_topn_probes(idx.h, C.byref(a1), C.byref(b1))
            probes = row["topn_probes_per_call"] = (a1.value - a0.value) // args.reps
            # the counter counts records.  Every probe of these shapes must be a top-n probe (a full-route record would come back as 12 bytes, not
            # 8); with the entries come the batch's tables: segment bounds (2 per probe + 1), buffer offsets (1 per probe + 1) and counts, u32 each
            assert probes == len(set(prefixes)) * parts, (probes, len(set(prefixes)), parts)
            row["bytes_back_per_call"] = (b1.value - b0.value) // args.reps * 8 + (4 * probes + 2) * 4
            idx.profile_enable()
            idx.profile_json()
            for _ in range(5):  # the kernels' device time in runs of their own (events on the stream slow the host side a little)
                run()
            prof = idx.profile_json()["kernels"]
            idx.profile_enable(False)
            row["device_ms_per_call"] = {k: round(prof.get(k, {}).get("ms", 0.0) / 5, 4) for k in ("k_dict_scan", "k_dict_topn<group>", "k_dict_topn")}
        else:
            row["bytes_back_per_call"] = matches * 12
        row["answers"] = [[list(e) for e in a] for a in answers]
        result["parts"][str(parts)] = row
    print("SUGGEST_BATCH_LEG " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "suggest_batch", "run"))
    ap.add_argument("--terms", default="300000,1000000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--leg")
    ap.add_argument("--child-terms", type=int)
    args = ap.parse_args()
    if args.leg:
        return child(args)
    if not args.parent_tree or not os.path.exists(os.path.join(args.parent_tree, "veloci_amd", "libveloci_amd.so")):
        sys.exit("--parent-tree: the parent commit, built, is the baseline of this measurement; check it out, build its library and pass its path")
    assert args.reps >= 20 and args.warmup >= 5
    os.makedirs(args.out, exist_ok=True)
    table = {}
    for terms in [int(t) for t in args.terms.split(",")]:
        legs = {}
        for leg in ("single", "batch"):
            env = dict(os.environ)
            env.pop("VQ_NO_SUGGEST_TOPN", None)
            env.pop("VQ_LIB", None)
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--child-terms", str(terms),
                   "--reps", str(args.reps), "--warmup", str(args.warmup)] + (["--tree", os.path.abspath(args.parent_tree)] if leg == "single" else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0 or "SUGGEST_BATCH_LEG " not in r.stdout:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit("leg %s over %d terms ended with status %d: nothing more is started" % (leg, terms, r.returncode))
            legs[leg] = json.loads(r.stdout.split("SUGGEST_BATCH_LEG ", 1)[1])
            print("done:", leg, terms, {p: (v["median_ms"], v["min_ms"], v["max_ms"]) for p, v in legs[leg]["parts"].items()}, flush=True)
        for parts in ("1", "3"):
            s, b = legs["single"]["parts"][parts], legs["batch"]["parts"][parts]
            same = s.pop("answers") == b.pop("answers")
            table["%d terms, %s part%s" % (terms, parts, "" if parts == "1" else "s")] = {"single_parent": s, "batch": b, "answers_equal": same,
                                                                                           "single_lib": legs["single"]["lib"], "batch_lib": legs["batch"]["lib"]}
    with open(os.path.join(args.out, "suggest_batch.json"), "w") as f:
        f.write(json.dumps(table, indent=1) + "\n")
    lines = ["| dictionary, parts | 256 single calls, parent: median (min - max) ms | one batch: median (min - max) ms | k_dict_scan / group / k_dict_topn ms | bytes back, single | bytes back, batch | equal |",
             "|---|---|---|---|---|---|---|"]
    for name, row in table.items():
        s, b = row["single_parent"], row["batch"]
        d = b["device_ms_per_call"]
        lines.append("| %s | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.3f / %.3f / %.3f | %d | %d | %s |" % (
            name, s["median_ms"], s["min_ms"], s["max_ms"], b["median_ms"], b["min_ms"], b["max_ms"], d["k_dict_scan"], d["k_dict_topn<group>"], d["k_dict_topn"],
            s["bytes_back_per_call"], b["bytes_back_per_call"], "yes" if row["answers_equal"] else "NO"))
    with open(os.path.join(args.out, "table.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
