"""Regex leaves on the device: k_dict_regex time per probe against the host route (usage: python tools/measure_dict_regex.py [out.json]).
300 000-term widecorpus dictionary (8 lowercase letters per term), the four patterns of the issue that introduced the kernel.  Per pattern: the
profiled k_dict_regex time of a request with that one leaf, the wall time of the request, and — from a child process with VQ_NO_REGEX_DEVICE=1
— the wall time of the same request on the host route (std::wregex over every term).  Then 16 distinct probes in one batch (the four patterns x
starts_with x two ignore_case settings), and a prefix probe's k_dict_scan time over the same dictionary: it reads the same bytes, the floor."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import veloci_amd  # noqa: E402
import widecorpus  # noqa: E402

PATTERNS = ["ab.*", "(foo|ba[rz])+x?", "[a-c]{2,3}d.*e", ".*[a-g]"]
HOST = os.environ.get("VQ_NO_REGEX_DEVICE") == "1"


def req(pattern, **kw):
    return {"search_req": {"search": dict({"path": "body", "terms": [pattern], "is_regex": True}, **kw)}, "top": 10}


def timed(idx, reqs, kernel):
    idx.profile_enable()
    idx.profile_json()
    t = time.perf_counter()
    res = veloci_amd.search_batch(reqs, idx)
    wall = (time.perf_counter() - t) * 1e3
    k = idx.profile_json()["kernels"].get(kernel, {})
    idx.profile_enable(False)
    return {"wall_ms": round(wall, 3), "kernel_ms": round(k.get("ms", 0.0), 4), "launches": k.get("launches", 0), "probes": k.get("queries", 0),
            "algorithmic_bytes": k.get("algorithmic_bytes", 0), "num_hits": [int(r.num_hits) for r in res]}


def main():
    data, terms = widecorpus.build(num_terms=300_000, num_docs=1_000_000, planted=False)
    idx = veloci_amd.Index(data, device=0)
    out = {"route": "host" if HOST else "device", "terms": len(terms), "patterns": {}}
    for p in PATTERNS:
        if not HOST:
            veloci_amd.search(req(p), idx)  # warm: code object, workspaces
            out["patterns"][p] = dict(timed(idx, [req(p)], "k_dict_regex"), route=idx.regex_route(req(p)["search_req"]["search"]))
        else:
            out["patterns"][p] = timed(idx, [req(p)], "k_dict_regex")
    if not HOST:
        sixteen = [req(p, **kw) for p in PATTERNS for kw in ({}, {"starts_with": True}, {"ignore_case": False}, {"ignore_case": False, "starts_with": True})]
        veloci_amd.search_batch(sixteen, idx)
        out["sixteen_probes"] = timed(idx, sixteen, "k_dict_regex")
        prefix = {"search_req": {"search": {"path": "body", "terms": ["ab"], "starts_with": True}}, "top": 10}
        veloci_amd.search(prefix, idx)
        out["prefix_probe_k_dict_scan"] = timed(idx, [prefix], "k_dict_scan")
        child = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, VQ_NO_REGEX_DEVICE="1"), capture_output=True, text=True, timeout=900)
        assert child.returncode == 0 and "DICT_REGEX " in child.stdout, child.stdout[-2000:] + child.stderr[-3000:]
        out["host_route"] = json.loads(child.stdout.split("DICT_REGEX ", 1)[1])["patterns"]
        for p in PATTERNS:
            assert out["host_route"][p]["num_hits"] == out["patterns"][p]["num_hits"], p
    line = "DICT_REGEX " + json.dumps(out)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
