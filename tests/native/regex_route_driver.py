"""Driver of the host-stub build for regex leaves on the device route (run by tests/test_regex_dfa_cpu.py with VQ_LIB=<host-stub library>,
VQ_STUB_NOOP_LAUNCH=1 and VQ_STUB_DICT_SCAN=1: the stubbed launch_dict_regex walks, on the host, the very tables k_dict_regex would read).
For every regex part below, over a wordcorpus dictionary and a hand-built non-ASCII one (Latin-1, Greek, Cyrillic, a code point above U+FFFF:
the u32 image): vq_debug_compile, vq_suggest_json and vq_highlight_json — term ids, scores, error texts — must equal what a child process of
this script gives with VQ_NO_REGEX_DEVICE=1 (the host route, std::wregex over every term); vq_debug_regex_compile reports the device route for
every part inside the compiler's grammar and the host route, with a reason, for the declined ones; an invalid pattern is the same error on
both routes.  Prints one summary line."""
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import numpy as np  # noqa: E402
import veloci_amd  # noqa: E402
import widecorpus  # noqa: E402
import wordcorpus  # noqa: E402
from veloci_amd import _lib  # noqa: E402

assert "host_stub" in _lib.lib_path(), _lib.lib_path()
assert os.environ.get("VQ_STUB_NOOP_LAUNCH") == "1" and os.environ.get("VQ_STUB_DICT_SCAN") == "1"
HOST_ONLY = os.environ.get("VQ_NO_REGEX_DEVICE") == "1"

WORD_PATTERNS = ["maj.*", "ma[gj].*", "(sea|see).*", "s[ae]{2}rch(es|ed)?", "the(ir|re|m)s?", ".*ner", "[a-c]{1,4}", r"\w+", r"\S*ß\S*", "straße", "STRASSE",
                 "ü.*", "привет.?", "[а-я]+", ".*京.*", "東京都?", "n[iI][eE]?c[eE]", "x?", "q{3}", ".*", "l[ai]t+?er", "(?:fe|le|wea)ther", "th[^e]+", r"\d+",
                 "ab?c?d?e?", "im+(er)?", ".+tt.+", "(a|b)+", "ma.{3,5}", "[^a-z]+", "(|maj)or", r"\W", "[äöüéèßñ]", "se*?a", r"majest\S{1,2}"]
WIDE_TERMS = ["a", "ab", "Éclair", "éclair", "ECLAIR", "straße", "STRASSE", "ΑΘΗΝΑ", "αθηνα", "Αθήνα", "σοφός", "ΣΟΦΟΣ", "привет", "ПРИВЕТ", "東京", "x\U0001F600y", "\U00010400\U00010428",
              "\U00010428", "µm", "μm", "ÿ", "Ÿ", "K", "k", "K", "line\nbreak", "tab\there", "q" * 300, "q" * 299 + "é", "zz9", "ß", "ǆ", "ǅ", "Ǆ"]
WIDE_PATTERNS = ["é.*", "É.*", ".*σ", ".*ς", "[α-ω]+", "[Α-Ω]+", "αθ.να", ".*\U0001F600.*", "\U00010400.?", "[\U00010400-\U0001044f]+", "µm|km", "μ.", "q{299}.", "q+",
                 r"\w+", r"\W+", r"\S+", ".", ".+", "k", "[k]", "ÿ", "[ÿ-ÿ]", "straße", r"line\nbreak", "line.break", r"\s", "ǆ", "п.*т", "[^a-z]{2}"]
DECLINED = [r"(a)\1", "ma(?=j)", "ma(?!j)", "^maj", "er$", r"\bsea", r"sea\B.", "[[:alpha:]]+", "a[]b", "a[^]b", ".*a.{13}", r"\x61", r"a\u0062"]
INVALID = ["ma(j", "[z-a]", "a{2,1}", "*a", "a{", "a\\", "[a"]


def parts_of(patterns):
    out = []
    for i, pat in enumerate(patterns):
        out.append({"path": "body", "terms": [pat], "is_regex": True})
        extra = [{"starts_with": True}, {"ignore_case": False}, {"ignore_case": True, "starts_with": True}, {"ignore_case": False, "starts_with": True}][i % 4]
        out.append(dict(out[-1], **extra))
    return out


def outcome(fn):
    try:
        return fn()
    except veloci_amd.VelociError as e:
        return "error: " + str(e)


def run_corpus(idx, parts):
    L = _lib.lib()
    rows = []
    for p in parts:
        req = veloci_amd.Request({"search_req": {"search": p}, "top": 10})
        row = {"compile": int(L.vq_debug_compile(idx.h, req.h))}
        row["suggest"] = outcome(lambda: veloci_amd.suggest(dict(p, top=1000), idx))
        row["highlight"] = outcome(lambda: veloci_amd.highlight(dict(p, snippet=True, top=1000), idx))
        rows.append(row)
    return rows


def main():
    word_data, word_terms = wordcorpus.build(num_docs=2000)
    rng = np.random.default_rng(3)
    wide_data, wide_terms = widecorpus.crafted(500, {t: rng.choice(500, size=int(rng.integers(1, 9)), replace=False) for t in WIDE_TERMS})
    corpora = [("words", veloci_amd.Index(word_data, device=0), parts_of(WORD_PATTERNS)), ("wide", veloci_amd.Index(wide_data, device=0), parts_of(WIDE_PATTERNS))]
    result = {"rows": {}, "routes": {}, "launches": 0, "probes": 0}
    for name, idx, parts in corpora:
        every = parts + parts_of(DECLINED)[::2] + parts_of(INVALID)[::2]
        result["rows"][name] = run_corpus(idx, every)
        # the profile counts the launches of searches: a batch of three leaves that match no term (a leaf of several terms would send the
        # stubbed device into k_union, whose host side sizes buffers by counts no launch wrote); results are garbage here, the probes are real
        idx.profile_enable()
        one = [{"search_req": {"search": {"path": "body", "terms": [t], "is_regex": True, "ignore_case": False}}, "top": 5} for t in ("q{3}z", "zq+z", "x{2}y{2}")]
        assert len(veloci_amd.search_batch(one + one[:1], idx)) == 4
        prof = idx.profile_json()["kernels"].get("k_dict_regex", {})
        result["launches"] += prof.get("launches", 0)
        result["probes"] += prof.get("queries", 0)
        routes = []
        for p in every:
            r = outcome(lambda: idx.regex_route(p))
            routes.append(r if isinstance(r, str) else ("device" if r["device"] else "host: " + r["reason"]))
        result["routes"][name] = routes
        result["n_parts"] = result.get("n_parts", 0) + len(parts)
        result.setdefault("n_in_grammar", {})[name] = len(parts)
    return result


if __name__ == "__main__":
    mine = main()
    if HOST_ONLY:
        assert mine["launches"] == 0, mine["launches"]
        assert all(r.startswith("host: ") or r.startswith("error: ") for rs in mine["routes"].values() for r in rs)
        print("REGEX_ROUTE_CHILD " + json.dumps(mine))
        sys.exit(0)
    child = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, VQ_NO_REGEX_DEVICE="1"), capture_output=True, text=True, timeout=600)
    assert child.returncode == 0 and "REGEX_ROUTE_CHILD " in child.stdout, child.stdout[-2000:] + child.stderr[-4000:]
    host = json.loads(child.stdout.split("REGEX_ROUTE_CHILD ", 1)[1])
    mine = json.loads(json.dumps(mine))  # tuples -> lists, as in the child's
    matched = 0
    for name in mine["rows"]:
        assert len(mine["rows"][name]) == len(host["rows"][name])
        n = mine["n_in_grammar"][name]
        for k, (a, b) in enumerate(zip(mine["rows"][name], host["rows"][name])):
            assert a == b, (name, k, a, b)
            matched += len(a["suggest"]) if isinstance(a["suggest"], list) else 0
        routes = mine["routes"][name]
        assert all(r == "device" for r in routes[:n]), [r for r in routes[:n] if r != "device"]
        assert all(r.startswith("host: ") and len(r) > 12 for r in routes[n:n + len(DECLINED)]), routes[n:n + len(DECLINED)]
        assert all(r.startswith("error: InvalidRequest: \"regex ") for r in routes[n + len(DECLINED):]), routes[n + len(DECLINED):]
        assert routes[n + len(DECLINED):] == host["routes"][name][n + len(DECLINED):]  # an invalid pattern: the same text on both routes
        # the invalid ones fail the same way through the search entry points
        for a in mine["rows"][name][n + len(DECLINED):]:
            assert a["compile"] == 1 and str(a["suggest"]).startswith("error: InvalidRequest: \"regex "), a  # 1: VQ_ERR_INVALID_REQUEST
    # per corpus one launch for the three distinct leaves of the profiled batch
    assert mine["probes"] == 6 and mine["launches"] == 2, (mine["probes"], mine["launches"])
    assert matched > 1000, matched
    print("REGEX_ROUTE_DRIVER_OK " + json.dumps({"parts": mine["n_parts"], "declined": len(DECLINED), "invalid": len(INVALID), "suggested_terms": matched,
                                                 "regex_launches": mine["launches"]}))
