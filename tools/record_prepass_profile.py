#!/usr/bin/env python3
"""Records tests/golden/prepass_profile.json: per pre-pass debug call and kernel, the launches and byte counts of the profile.  Run it on an
MI355X with the library of the commit whose device work is to be pinned (tests/test_gpu_prepass_profile.py makes the same calls and compares).

    python tools/record_prepass_profile.py [out.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("VQ_PROBE_MIN_DOCS", "0")  # as tests/conftest.py

from prepass_profile_calls import profile_calls  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "prepass_profile.json")
    with open(out, "w") as f:
        json.dump(profile_calls(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
