"""Doc sets ordered by a column (vq_docset_top_by, DocSet.top_by) without a GPU: the assertion that the shared cases are not vacuous, the whole
host path over the stubbed device layer against the yardstick (tests/native/docset_top_driver.py, tests/docsettopcases.py), the same host code
under ASan + UBSan as a program of its own (tests/native/docset_top_check.cpp), the compiler's resource report of docset_top.hip, and the places
that must name the new entry point."""
import json
import os
import re
import subprocess
import sys

import pytest

import docsettopcases as TC
import sanitized
import test_kernel_resources as KR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "veloci_amd", "csrc")


def test_the_cases_reach_every_image_kind_tie_cuts_chunks_classes_and_the_lowest_byte():
    seen = TC.assert_not_vacuous()
    print(seen)
    assert seen["kinds"] == ["dense", "empty", "plain", "tiled"]
    for name in ("cut-inside-run", "cut-at-run-end", "run-over-chunks", "threshold-nan", "threshold-missing", "lowest-byte", "1n-several", "select", "all-winners"):
        assert seen[name] > 0, (name, seen)
    header = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert "constexpr uint32_t kTopMaxRows = %d;" % TC.MAX_ROWS in header
    assert max(t + s for _, _, t, s, _, _ in TC.cases()) == TC.MAX_ROWS


def test_top_by_on_the_stubbed_device_equals_the_yardstick():
    r = subprocess.run(["make", "-C", CSRC, "-j6", "hoststub"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    env = dict(os.environ, VQ_LIB=os.path.join(ROOT, "veloci_amd", "_host_stub", "libveloci_host_stub.so"), VQ_STUB_DICT_SCAN="1", VQ_HOST_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(HERE, "native", "docset_top_driver.py")], capture_output=True, text=True, timeout=900, env=env)
    tail = r.stdout[-1500:] + r.stderr[-6000:]
    assert r.returncode == 0 and "DOCSET_TOP_DRIVER_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_TOP_DRIVER_OK ", 1)[1])
    print(stats)
    assert stats["cases"] == len(TC.cases()) and stats["strided"] == stats["forced"] > 1000 and stats["merges"] == 3 * len(TC.shard_cases()), stats


def test_top_by_merge_pack_and_unpack_under_asan_and_ubsan(tmp_path):
    host_srcs, stubs = sanitized.host_sources()
    assert any(s.endswith("hip_stub_docset_top.cpp") for s in stubs) and "docset_top.cpp" in host_srcs
    r, tail = sanitized.run(sanitized.build_host_check(tmp_path, "docset_top_check", host_srcs, stubs))
    assert r.returncode == 0 and "DOCSET_TOP_CHECK_OK " in r.stdout, tail
    stats = json.loads(r.stdout.split("DOCSET_TOP_CHECK_OK ", 1)[1])
    print(stats)
    assert stats["calls"] > 1000 and stats["merges"] == 3 * 3 * 2 * 2 * 2, stats


@pytest.mark.skipif(KR.HIPCC is None, reason="no hipcc")
def test_the_top_kernels_compile_for_gfx950_without_scratch(tmp_path):
    rows = {k: v for k, v in KR.resource_report("docset_top.hip", tmp_path).items() if "k_top_" in k}
    print(rows)
    names = ("k_top_fold", "k_top_keys", "k_top_pick", "k_top_hist", "k_top_tiecount", "k_top_emit")
    assert len(rows) == len(names) and all(sum(n in k for k in rows) == 1 for n in names), sorted(rows)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k, v in rows.items():  # the line the other doc-set kernels are held to
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs"] + v.get("AGPRs", 0) <= 64, (k, v)
        name = next(n for n in names if n in k)
        stated = re.search(r"`%s`[^|\n]*\| *(\d+) B of LDS" % name, design)  # the kernel table of DESIGN.md
        assert stated, name
        assert v["LDS Size [bytes/block]"] == int(stated.group(1)) == (1024 if name in ("k_top_keys", "k_top_hist") else 0), (k, v, stated.group(1))


def test_every_layer_names_the_entry_point():
    symbols = ("vq_docset_top_by", "vq_docset_top_len", "vq_docset_top_docs", "vq_docset_top_values", "vq_docset_top_kinds", "vq_docset_top_counters", "vq_docset_top_is_partial",
               "vq_docset_top_merge", "vq_docset_top_pack", "vq_docset_top_unpack", "vq_docset_top_free", "vq_debug_docset_top_ms")
    for rel in ("include/veloci_amd.h", "veloci_amd/_lib.py", "INTEGRATION.md", "veloci_amd/csrc/capi.cpp"):
        text = open(os.path.join(ROOT, rel)).read()
        for name in symbols:
            assert name in text, (rel, name)
    for rel in ("DESIGN.md", "README.md"):
        assert "vq_docset_top_by" in open(os.path.join(ROOT, rel)).read(), rel
    py = open(os.path.join(ROOT, "veloci_amd", "search.py")).read()
    for name in ("def top_by(self, field, top=10, skip=0, descending=False, with_missing=True)", "def merge_top_by(parts)", "class TopByResult", "def pack(self)"):
        assert name in py, name
    assert "def top_by_shards_local(shards, sets, field, **kw)" in open(os.path.join(ROOT, "veloci_amd", "dist.py")).read()
    import veloci_amd
    assert callable(veloci_amd.merge_top_by) and hasattr(veloci_amd.DocSet, "top_by")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = mk.split("SRCS =", 1)[1].split("\n", 1)[0].split()
    assert "docset_top.hip" in srcs and "docset_top.cpp" in srcs and "docset_top.cpp" in mk.split("HOST_SRCS =", 1)[1].split("\n", 1)[0].split()
    kernels = open(os.path.join(CSRC, "kernels.hpp")).read()
    for name in ("launch_top_fold", "launch_top_keys", "launch_top_pick", "launch_top_hist", "launch_top_tiecount", "launch_top_emit", "struct DocsetTopD", "kTopMaxRows"):
        assert name in kernels, name
    # the column resolution is shared with from_ranges and the aggregations, not copied
    top = open(os.path.join(CSRC, "docset_top.cpp")).read()
    assert "resolve_range_column(" in top and "BOOST_VALID_TO_VALUE" not in top and open(os.path.join(CSRC, "docset_ranges.cpp")).read().count("resolve_range_column(") == 2
    # hist_add is defined once, in the shared header, and both selects use it
    defined = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".hip", ".hpp")) and "void hist_add(" in open(os.path.join(CSRC, fn)).read()]
    assert defined == ["kernel_common.hpp"], defined
    assert "hist_add(" in open(os.path.join(CSRC, "text_rank.hip")).read() and "hist_add(" in open(os.path.join(CSRC, "docset_top.hip")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("k_top_fold", "k_top_keys", "k_top_pick", "k_top_hist", "k_top_tiecount", "k_top_emit", "docset_top.hip", "docset_top.cpp", "vq_docset_top_merge", "kTopMaxRows"):
        assert name in design, name
    knobs = design.split("8a", 1)[1] if "8a" in design else ""
    assert "VQ_TOP_MAX_GRID" in knobs and "VQ_TOP_FORCE_SELECT" in knobs
    header = open(os.path.join(ROOT, "include", "veloci_amd.h")).read()
    assert "VQ_TOP_MAX_GRID" in header and "VQ_TOP_FORCE_SELECT" in header
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ds.top_by(" in readme
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "DocSet.top_by" in integration and "vq_docset_top_unpack" in integration and "all-gather" in integration
