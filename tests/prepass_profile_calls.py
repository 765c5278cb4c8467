"""One call per pre-pass debug entry point on the corpora of tests/test_gpu_prepass_lists.py, each followed by profile_json(reset=True): what the
runners launched and the byte counts they booked, kernel by kernel.  Shared by tests/test_gpu_prepass_profile.py (which compares with
tests/golden/prepass_profile.json) and tools/record_prepass_profile.py (which writes that file)."""
import numpy as np

import prepasscorpus as P
import test_gpu_prepass_lists as T

FIELDS = ("launches", "layout_bytes", "algorithmic_bytes", "queries")


def _range_jobs(u):
    """both paths of k_range_hits in one call: one list with 130 anchors (a lane per anchor), 65 lists (a workgroup per anchor), jobs without work"""
    rng = np.random.default_rng(7)
    docs = u.lists[u.edge][0]
    pool_docs = np.unique(np.concatenate([u.lists[t][0] for t in u.pool[:65]]))
    return [([u.edge], T.anchors_around(rng, docs, 130)), ([], [3, 9, 27]), (u.pool[:65], T.anchors_around(rng, pool_docs, 5)), ([u.big[0]], []),
            (u.big[:3], T.anchors_around(rng, u.lists[u.big[2]][0], 64))]


def profile_calls():
    """-> {call name: {kernel: {field: int}}}"""
    u, l, b = T.UnionCorpus(), T.LocalityCorpus(), T.Boost1nCorpus()
    out = {}

    def take(name, idx, rc):
        assert rc == 0, (name, rc)
        kernels = idx.profile_json(reset=True)["kernels"]
        out[name] = {k: {f: int(v[f]) for f in FIELDS} for k, v in sorted(kernels.items())}

    idx = T.open_index(u.data)
    two = u.groups()["two_levels"]
    idx.profile_json(reset=True)
    take("union_two_levels", idx, P.run_union(idx, two, 1)[0])
    take("union_dense", idx, P.run_union(idx, two, 2)[0])
    take("range_hits_both_paths", idx, P.run_range_hits(idx, _range_jobs(u))[0])
    idx.close()

    idx = T.open_index(l.data)
    idx.profile_json(reset=True)
    take("locality_two_tables", idx, P.run_locality(idx, [l.jobs[n] for n in T.ALL_17])[0])
    idx.close()

    idx = T.open_index(b.data)
    idx.profile_json(reset=True)
    take("boost1n", idx, P.run_boost1n(idx, [b.jobs[n] for n in sorted(b.jobs)])[0])
    idx.close()
    return out
