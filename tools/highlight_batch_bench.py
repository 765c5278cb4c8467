"""Batched highlight against a loop of single highlights (needs a GPU).

    python tools/highlight_batch_bench.py --parent-tree <checkout of the parent commit, library built> [--out DIR, default profiles/highlight_batch/run]

256 parts of the reference generator's shape (starts_with, snippet, top 10, skip 0) on one tokenized field of 300 000 texts, eight words
each, over 20 000 words of eight lowercase letters whose first letter is one of four; the two-letter word `ab` is in more than half of the
texts and is the best match of the prefix `a`, the other words follow a skewed distribution.  Prefixes of 1, 2, 3 and 5 letters in equal parts.
Two legs, each in a child process of its own under `timeout`:
  single   a loop of 256 vq_highlight_json calls on the PARENT commit (--parent-tree: its Python package and its library): the baseline
  batch    one vq_highlight_batch call on this tree's library
Per leg: the median, minimum and maximum wall time of the repetitions after the warm-ups (the first batch also checks the field's stores).
For the batch also device_parts and snippets_built per call (vq_index_highlight_rank_counts), and the device time per call of k_dict_scan,
k_text_best and k_text_select from vq_profile_json.  The answers of both legs are compared.  Writes highlight_batch.json into --out; after a child that fails or runs into its time limit nothing
more is started."""
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

N_PARTS = 256
N_TEXTS = 300_000
N_WORDS = 20_000
WORDS_PER_TEXT = 8
FIELD = "body"


def build():
    """-> (IndexData, sorted word list, per-word text counts)"""
    import numpy as np
    from veloci_amd.index import IndexData
    rng = np.random.default_rng(77)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)
    raw = letters[rng.integers(0, 26, size=(N_WORDS, 8))]
    raw[:, 0] = letters[rng.integers(0, 4, size=N_WORDS)]
    words = sorted({bytes(r) for r in raw} | {b"ab"})
    terms = [b" "] + words  # bytewise order: the separator first
    n_terms = len(terms)
    frequent = terms.index(b"ab")
    # word ids of every text: a skewed draw (the square of a uniform), `ab` in the first place of 55 % of the texts
    picks = 1 + (rng.random((N_TEXTS, WORDS_PER_TEXT)) ** 2 * len(words)).astype(np.int64)
    picks[rng.random(N_TEXTS) < 0.55, 0] = frequent
    rows = np.zeros((N_TEXTS, 2 * WORDS_PER_TEXT - 1), np.uint32)  # word, separator, word, ...
    rows[:, 0::2] = picks
    text_ids = n_terms + 1 + np.arange(N_TEXTS, dtype=np.uint64)   # texts too long for the dictionary: ids behind it
    pairs = np.unique(rows.astype(np.uint64).ravel() * (1 << 32) + np.repeat(text_ids, rows.shape[1]))
    tok = (pairs >> 32).astype(np.int64)
    counts = np.bincount(tok, minlength=n_terms)
    t2t_off = np.zeros(n_terms + 1, np.uint64)
    t2t_off[1:] = np.cumsum(counts)
    data = IndexData(N_TEXTS)
    path = FIELD + ".textindex"
    data.add_fst(path, terms)
    data.set_column_meta(FIELD, False, True)
    one = np.arange(n_terms + 1, dtype=np.uint64)
    anchors = (np.arange(n_terms) % N_TEXTS).astype(np.uint32)
    data.add_token_to_anchor_score(path + ".to_anchor_id_score", one, anchors, np.full(n_terms, 10, np.uint32), None)
    data.add_key_value_store(path + ".text_id_to_anchor", one, anchors)
    data.add_key_value_store(path + ".tokens_to_text_id", t2t_off, (pairs & 0xFFFFFFFF).astype(np.uint32))
    data.add_key_value_store(path + ".text_id_to_token_ids", np.arange(N_TEXTS + 1, dtype=np.uint64) * rows.shape[1], rows.ravel(), key_base=int(text_ids[0]))
    assert counts[frequent] * 2 >= N_TEXTS, counts[frequent]
    return data, words, counts[1:]


def parts_of(words):
    import numpy as np
    rng = np.random.default_rng(2024)
    out = []
    for n_letters in (1, 2, 3, 5):
        for t in rng.integers(0, len(words), size=N_PARTS // 4):
            out.append({"path": FIELD, "terms": [words[int(t)].decode()[:n_letters]], "starts_with": True, "levenshtein_distance": 0, "snippet": True, "top": 10, "skip": 0})
    return out


def child(args):
    if args.tree:  # the parent commit's package and library instead of this tree's
        sys.path.insert(0, os.path.abspath(args.tree))
    import veloci_amd
    from veloci_amd import _lib
    data, words, counts = build()
    idx = veloci_amd.Index(data, device=0)
    assert os.path.abspath(_lib.lib_path()).startswith(os.path.abspath(args.tree or ROOT)), _lib.lib_path()
    parts = [json.dumps(p) for p in parts_of(words)]
    result = {"leg": args.leg, "lib": os.path.relpath(_lib.lib_path(), os.path.abspath(args.tree or ROOT)), "texts": N_TEXTS, "words": len(words),
              "texts_with_the_frequent_word": int(counts[words.index(b"ab")])}
    if args.leg == "single":
        run = lambda: [veloci_amd.highlight(p, idx) for p in parts]  # noqa: E731
    else:
        run = lambda: veloci_amd.highlight_batch(parts, idx)  # noqa: E731

    def counters():
        a, b = C.c_uint64(), C.c_uint64()
        _lib.lib().vq_index_highlight_rank_counts(idx.h, C.byref(a), C.byref(b))
        return a.value, b.value
    t = time.perf_counter()
    for _ in range(args.warmup):
        answers = run()
    result["warmup_ms"] = round((time.perf_counter() - t) * 1e3, 1)
    before = counters() if args.leg == "batch" else None
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        answers = run()
        times.append((time.perf_counter() - t) * 1e3)
    result.update(median_ms=round(statistics.median(times), 3), min_ms=round(min(times), 3), max_ms=round(max(times), 3), reps=len(times))
    if args.leg == "batch":
        after = counters()
        result["device_parts_per_call"] = (after[0] - before[0]) // args.reps
        result["snippets_built_per_call"] = (after[1] - before[1]) // args.reps
        idx.profile_enable()
        idx.profile_json()
        for _ in range(3):  # the kernels' device time in runs of their own (events on the stream slow the host side a little)
            run()
        prof = idx.profile_json()["kernels"]
        idx.profile_enable(False)
        result["device_ms_per_call"] = {k: round(prof.get(k, {}).get("ms", 0.0) / 3, 4) for k in ("k_dict_scan", "k_text_best", "k_text_select")}
    result["entries"] = sum(len(a) for a in answers)
    result["answers"] = [[list(e) for e in a] for a in answers]
    print("HIGHLIGHT_BATCH_LEG " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "highlight_batch", "run"))
    ap.add_argument("--reps-single", type=int, default=3)
    ap.add_argument("--reps-batch", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--leg")
    ap.add_argument("--reps", type=int)
    ap.add_argument("--warmup", type=int)
    args = ap.parse_args()
    if args.leg:
        return child(args)
    if not args.parent_tree or not os.path.exists(os.path.join(args.parent_tree, "veloci_amd", "libveloci_amd.so")):
        sys.exit("--parent-tree: the parent commit, built, is the baseline of this measurement; check it out, build its library and pass its path")
    os.makedirs(args.out, exist_ok=True)
    legs = {}
    for leg in ("single", "batch"):
        env = dict(os.environ)
        env.pop("VQ_NO_HIGHLIGHT_RANK", None)
        env.pop("VQ_LIB", None)
        reps, warmup = (args.reps_single, 1) if leg == "single" else (args.reps_batch, 3)
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--reps", str(reps), "--warmup", str(warmup)]
        cmd += ["--tree", os.path.abspath(args.parent_tree)] if leg == "single" else []
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        if r.returncode != 0 or "HIGHLIGHT_BATCH_LEG " not in r.stdout:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("leg %s ended with status %d: nothing more is started" % (leg, r.returncode))
        legs[leg] = json.loads(r.stdout.split("HIGHLIGHT_BATCH_LEG ", 1)[1])
        print("done:", leg, {k: v for k, v in legs[leg].items() if k != "answers"}, flush=True)
    same = legs["single"].pop("answers") == legs["batch"].pop("answers")
    table = {"single_parent": legs["single"], "batch": legs["batch"], "answers_equal": same}
    with open(os.path.join(args.out, "highlight_batch.json"), "w") as f:
        f.write(json.dumps(table, indent=1) + "\n")
    s, b = legs["single"], legs["batch"]
    print("256 single calls on the parent: %.1f (%.1f - %.1f) ms; one batch: %.2f (%.2f - %.2f) ms; snippets built per batch: %d; answers equal: %s" % (
        s["median_ms"], s["min_ms"], s["max_ms"], b["median_ms"], b["min_ms"], b["max_ms"], b["snippets_built_per_call"], "yes" if same else "NO"))


if __name__ == "__main__":
    main()
