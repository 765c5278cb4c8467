"""Generates tests/golden/log_vectors.json: f32 inputs with their exactly rounded f32 log10 / log2, computed with mpmath at 200 bits (nothing
of the product, the oracle or tests/boostref.py's long-double route runs here — the file anchors that route, tests/test_boost_ref_cpu.py).
Inputs: the structured finite inputs of boostref (around 1, the exact powers of ten and two, denormals, FLT_MAX) and seeded random positive
bit patterns, 2048 in all.  The tests read the JSON only; mpmath is needed here alone.  Run from the repo root: python tests/gen_log_vectors.py"""
import json
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import boostref  # noqa: E402  (its input lists only)

COUNT = 2048
SEED = 77003


def exact_f32_bits(x, base):
    """bit pattern of log_base(x) rounded to nearest-even f32; x a positive finite f32.  The result is 0 or a normal f32 (|log| >= 5e-8), so
    rounding the 200-bit value to 24 bits is the f32 rounding; at 200 bits no result that is not exact comes near a midpoint."""
    with mpmath.workprec(200):
        y = mpmath.log(mpmath.mpf(float(x)), base)  # (float(x) is exact: every f32 is an f64)
        with mpmath.workprec(24):
            r = +y  # rounds to nearest even
        f = np.float32(float(r))
        assert mpmath.mpf(float(f)) == r
    return int(f.view(np.uint32))


def main():
    xs = list(boostref.structured_inputs())
    rng = np.random.default_rng(SEED)
    xs += list(boostref.from_bits(rng.integers(1, 0x7F800000, COUNT - len(xs), dtype=np.uint32)))
    xs = np.array(xs, np.float32)
    assert len(xs) == COUNT and np.all(xs > 0) and np.all(np.isfinite(xs))
    doc = {"comment": "f32 bit patterns: x, and log10(x) / log2(x) rounded to nearest-even f32 from mpmath at 200 bits (tests/gen_log_vectors.py)",
           "x_bits": ["%08x" % int(b) for b in boostref.bits(xs)],
           "log10_bits": ["%08x" % exact_f32_bits(x, 10) for x in xs],
           "log2_bits": ["%08x" % exact_f32_bits(x, 2) for x in xs]}
    with open(os.path.join(HERE, "golden", "log_vectors.json"), "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("wrote", len(xs), "vectors")


if __name__ == "__main__":
    main()
