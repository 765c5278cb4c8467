"""Host-side mirror of the reference's search surface (src/search.rs:143, src/search/request/mod.rs,
src/search/result/search_result.rs) over the C ABI: `search(request, index) -> SearchResult`."""
import ctypes as C
import json

import numpy as np

from . import _lib
from ._lib import VelociError  # noqa: F401  (re-exported)


class Hit:
    """search::Hit (src/search.rs:53-57)."""
    __slots__ = ("id", "score")

    def __init__(self, id, score):
        self.id = int(id)
        self.score = float(score)

    def __repr__(self):
        return f"Hit(id={self.id}, score={self.score!r})"

    def __eq__(self, o):
        return isinstance(o, Hit) and self.id == o.id and self.score == o.score


class SearchResult:
    """search::SearchResult (src/search/result/search_result.rs:9-26)."""

    def __init__(self, num_hits, ids, scores, facets, execution_time_ns):
        self.num_hits = int(num_hits)
        self.ids = ids              # np.uint32
        self.scores = scores        # np.float32
        self.facets = facets        # None or {field: [(value, count)]}
        self.execution_time_ns = int(execution_time_ns)
        self.is_page = False

    @property
    def data(self):
        return [Hit(i, s) for i, s in zip(self.ids.tolist(), self.scores.tolist())]

    def __repr__(self):
        return f"SearchResult(num_hits={self.num_hits}, data={self.data[:3]}..., facets={self.facets})"


class DocSet:
    """A set of anchor ids staged on the index's GPU (`vq_docset`).  Attached to a request it restricts the search to the set's docs, exactly as
    a `filter` leaf whose hits are these ids would (and-ed with the request's own `filter`).  `ids`: a numpy array or sequence of non-negative
    ints (copied as uint32; any order, duplicates allowed), or a contiguous torch tensor of dtype int32 / uint32 on the index's device (read in
    place, no host copy).  Immutable; any number of requests may share one, and a request keeps its set alive after `close()`.  Sets of one index
    compose on the device: `a & b`, `a | b`, `a - b`, `~a`, `a.minus(*others)`, `DocSet.combine` / `all_of` / `any_of` each make a new DocSet."""

    OPS = {"and": 0, "or": 1, "minus": 2, "not": 3}  # VQ_DOCSET_AND ...

    def __init__(self, index, ids):
        self.L = _lib.lib()
        self.h = None
        self.index = index  # the operators need it
        on_device, keep = 0, None
        if type(ids).__module__.split(".")[0] == "torch":
            import torch
            if ids.dtype not in (torch.int32, torch.uint32) or not ids.is_contiguous() or ids.dim() != 1:
                raise ValueError("DocSet: a torch tensor of ids must be one-dimensional, contiguous and of dtype int32 or uint32")
            if ids.is_cuda:
                if ids.device.index != index.device:
                    raise ValueError("DocSet: the ids tensor is not on the index's device")
                torch.cuda.current_stream(ids.device).synchronize()  # the library reads the ids on a stream of its own
                on_device, keep, ptr, n = 1, ids, ids.data_ptr(), ids.numel()
            else:
                ids = ids.numpy()
        if not on_device:
            arr = np.asarray(ids)
            if arr.size and arr.dtype.kind not in "iu":
                raise ValueError("DocSet: ids must be integers")
            if arr.size and (int(arr.min()) < 0 or int(arr.max()) > 0xFFFFFFFF):
                raise ValueError("DocSet: ids must fit an unsigned 32-bit integer")
            keep = np.ascontiguousarray(arr.reshape(-1), dtype=np.uint32)
            ptr, n = keep.ctypes.data, keep.size
        h = C.c_void_p()
        _lib.check(self.L.vq_docset_create(index.h, C.c_void_p(ptr) if n else None, n, on_device, C.byref(h)))
        self.h = h
        del keep

    @classmethod
    def from_filter(cls, index, filter, within=None):
        """The set of the docs a filter tree selects (`vq_docset_from_filter`), evaluated once on the index's GPU.  `filter`: what `Request.filter`
        holds, as a dict or JSON text (str / bytes); `within`: a DocSet of the same index that is and-ed in.  The ids are exactly those the filter of a
        request with this `filter` and doc set `within` selects, so `search(r, index, docset=DocSet.from_filter(index, f))` answers what `search`
        answers for `r` with `filter: f`.  On a shard the length is summed over the shards through `index.set_allreduce`'s hook."""
        if isinstance(filter, dict):
            filter = json.dumps(filter)
        if isinstance(filter, str):
            filter = filter.encode()
        self = cls.__new__(cls)
        self.L = _lib.lib()
        self.h = None
        self.index = index
        h = C.c_void_p()
        _lib.check(self.L.vq_docset_from_filter(index.h, filter, len(filter), within._handle() if within is not None else None, C.byref(h)))
        self.h = h
        return self

    @classmethod
    def from_ranges(cls, index, ranges, within=None):
        """The set of the docs whose numeric column values satisfy every clause (`vq_docset_from_ranges`), selected on the index's GPU.  `ranges`: a
        non-empty list of dicts or JSON text, e.g. [{"field": "price", "gte": 10, "lt": 100}, {"field": "rating", "gt": 4.5, "missing": True}]:
        `field` names the column `<field>.boost_valid_to_value`, at most one of gt / gte and one of lt / lte bound it, `missing` says whether a doc
        without a value satisfies the clause.  A stored f32 value is compared as a float64 with the bound as given; NaN satisfies no clause.  A
        field with "[]" holds when any of the doc's values does.  `within`: a DocSet of the same index that is and-ed in; one without a bitmap (a
        short candidate list) is probed id by id, so the cost follows it.  OR and NOT are `combine`'s.  The result is an ordinary DocSet.  On a
        shard the length is summed over the shards through `index.set_allreduce`'s hook."""
        if not isinstance(ranges, (str, bytes)):
            ranges = json.dumps(list(ranges), allow_nan=False)  # (JSON has no infinity: a bound beyond the floats goes in as text, e.g. 1e999)
        if isinstance(ranges, str):
            ranges = ranges.encode()
        self = cls.__new__(cls)
        self.L = _lib.lib()
        self.h = None
        self.index = index
        h = C.c_void_p()
        _lib.check(self.L.vq_docset_from_ranges(index.h, ranges, len(ranges), within._handle() if within is not None else None, C.byref(h)))
        self.h = h
        return self

    @classmethod
    def from_range(cls, index, field, gte=None, gt=None, lte=None, lt=None, missing=False, within=None):
        """`from_ranges` with one clause: DocSet.from_range(index, "price", gte=10, lt=100)"""
        clause = {"field": field, "missing": bool(missing)}
        clause.update({k: v for k, v in (("gte", gte), ("gt", gt), ("lte", lte), ("lt", lt)) if v is not None})
        return cls.from_ranges(index, [clause], within=within)

    @property
    def range_route(self):
        """vq_debug_docset_range_route: -1 the set was not made from ranges, 0 the stream route built it, 1 the probe route"""
        return int(self.L.vq_debug_docset_range_route(self._handle()))

    @classmethod
    def combine(cls, index, op, sets):
        """Set algebra on the index's GPU (`vq_docset_combine`): `op` "and" / "or" over one or more DocSets of `index`, "minus" (sets[0] without the
        ids of the others), "not" (one set: every anchor of the index's doc range outside it).  Any number of operands.  The result is an ordinary
        DocSet; the operands are only read and may be closed afterwards.  On a shard the length is summed through `index.set_allreduce`'s hook."""
        if op not in cls.OPS:
            raise ValueError('DocSet.combine: op must be "and", "or", "minus" or "not"')
        sets = list(sets)
        handles = (C.c_void_p * max(len(sets), 1))(*[s._handle() for s in sets])
        self = cls.__new__(cls)
        self.L = _lib.lib()
        self.h = None
        self.index = index
        h = C.c_void_p()
        _lib.check(self.L.vq_docset_combine(index.h, cls.OPS[op], handles, len(sets), C.byref(h)))
        self.h = h
        return self

    @classmethod
    def all_of(cls, index, sets):
        """the ids every one of `sets` holds"""
        return cls.combine(index, "and", sets)

    @classmethod
    def any_of(cls, index, sets):
        """the ids at least one of `sets` holds"""
        return cls.combine(index, "or", sets)

    def minus(self, *others):
        """this set without the ids of any of `others`"""
        return DocSet.combine(self.index, "minus", [self, *others])

    def __and__(self, other):
        return DocSet.combine(self.index, "and", [self, other]) if isinstance(other, DocSet) else NotImplemented

    def __or__(self, other):
        return DocSet.combine(self.index, "or", [self, other]) if isinstance(other, DocSet) else NotImplemented

    def __sub__(self, other):
        return DocSet.combine(self.index, "minus", [self, other]) if isinstance(other, DocSet) else NotImplemented

    def __invert__(self):
        return DocSet.combine(self.index, "not", [self])

    @property
    def route(self):
        """vq_debug_docset_route: -1 no combine made the set, 0 the word route built it, 1 the probe route"""
        return int(self.L.vq_debug_docset_route(self._handle()))

    def _handle(self):
        if not self.h:
            raise ValueError("DocSet: used after close()")
        return self.h

    def __len__(self):
        """unique ids of the whole set (the same on every shard)"""
        return int(self.L.vq_docset_len(self._handle()))

    @property
    def local_len(self):
        """those inside the index's doc range"""
        return int(self.L.vq_docset_local_len(self._handle()))

    @property
    def device_bytes(self):
        return int(self.L.vq_docset_device_bytes(self._handle()))

    def part(self, which):
        """vq_debug_docset_part: 0 the local ids, 1 bitmap words, 2 rank directory, 3 tile directory, 4 the local ids with their padding (numpy uint32;
        empty when the set carries no such part)"""
        n = int(self.L.vq_debug_docset_part(self._handle(), which, None, 0))
        out = np.zeros(n, np.uint32)
        if n:
            self.L.vq_debug_docset_part(self._handle(), which, out.ctypes.data_as(C.c_void_p), n)
        return out

    def ids(self):
        """the set's ids inside the index's doc range, sorted and unique (numpy uint32)"""
        return self.part(0)

    def ids_tensor(self):
        """the same ids as a torch int32 tensor on the index's device (`vq_docset_ids`, device to device: no host copy)"""
        import torch
        h, n = self._handle(), self.local_len
        dev = torch.device("cuda", self.index.device)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        if n:
            torch.cuda.current_stream(dev).synchronize()  # the library copies on a stream of its own: nothing of torch's may still use the memory
            if int(self.L.vq_docset_ids(h, C.c_void_p(out.data_ptr()), n, 1)) != n:
                raise VelociError(5, self.L.vq_last_error().decode() or "vq_docset_ids failed")
        return out

    def facet_result(self, facets):
        """The facet counts of the set's docs (`vq_docset_facets`) as a SearchResult: `num_hits` = len(self), no hits, `facets` as a search over
        exactly these docs reports them.  `facets`: what `Request.facets` holds, a list of dicts ({"field": .., "top": ..}) or JSON text.  Counted
        on the index's GPU without a search; on a shard the counts are summed over the shards through `index.set_allreduce`'s hook."""
        if not isinstance(facets, (str, bytes)):
            facets = json.dumps(list(facets))
        if isinstance(facets, str):
            facets = facets.encode()
        out = C.c_void_p()
        _lib.check(self.L.vq_docset_facets(self.index.h, self._handle(), facets, len(facets), C.byref(out)))
        return _take_result(self.L, out)

    def facets(self, facets):
        """-> {field: [(value, count)]}, the form of `SearchResult.facets` (None for an empty facet list); see `facet_result`"""
        return self.facet_result(facets).facets

    def aggregate(self, specs):
        """Numeric aggregations of the set's docs (`vq_docset_aggregate`), computed on the index's GPU.  `specs`: a non-empty list of
        {"field": "price"} or {"field": "price", "edges": [0, 10, 100]} (or JSON text).  -> one dict per spec, in request order: `docs` (len(self)),
        `count` (present non-NaN values), `missing` (docs without a value), `nan`, `min`, `max` (None when count == 0), `sum` (the exact sum of the
        finite values rounded once to float64: math.fsum's answer, the same on every run and sharding; +-inf / NaN by the infinities counted) and,
        with `edges`, `buckets`: len(edges) + 1 ints, bucket i counting e(i-1) <= v < e(i) as `from_range(gte=, lt=)` compares.  On a shard every
        rank gets the whole set's answer through `index.set_allreduce`'s hook."""
        if not isinstance(specs, (str, bytes)):
            specs = json.dumps(list(specs), allow_nan=False)  # (JSON has no infinity: an edge beyond the floats goes in as text, e.g. 1e999)
        if isinstance(specs, str):
            specs = specs.encode()
        h = C.c_void_p()
        _lib.check(self.L.vq_docset_aggregate(self.index.h, self._handle(), specs, len(specs), C.byref(h)))
        try:
            out = []
            for i in range(int(self.L.vq_docset_aggs_len(h))):
                a = self.L.vq_docset_aggs_get(h, i).contents
                d = {"docs": int(a.docs), "count": int(a.count), "missing": int(a.missing), "nan": int(a.nan), "min": float(a.min) if a.count else None,
                     "max": float(a.max) if a.count else None, "sum": float(a.sum)}
                if a.n_buckets:
                    d["buckets"] = [int(a.buckets[b]) for b in range(int(a.n_buckets))]
                out.append(d)
            return out
        finally:
            self.L.vq_docset_aggs_free(h)

    def stats(self, field):
        """-> dict(docs, count, missing, nan, min, max, sum, mean) of one column over the set; min, max and mean are None when count == 0"""
        d = self.aggregate([{"field": field}])[0]
        d["mean"] = d["sum"] / d["count"] if d["count"] else None
        return d

    def histogram(self, field, edges):
        """-> len(edges) + 1 ints: the set's values of `field` below edges[0], in [edges[i-1], edges[i]), at or above edges[-1]"""
        return self.aggregate([{"field": field, "edges": [float(e) for e in edges]}])[0]["buckets"]

    def top_by(self, field, top=10, skip=0, descending=False, with_missing=True):
        """Rows [skip, skip + top) of the set's docs ordered by the column `<field>.boost_valid_to_value` (`vq_docset_top_by`), selected on the
        index's GPU -> TopByResult.  The order: docs with a number by value (ascending, or descending), then docs whose value is NaN, then docs
        without a value, ties (-0 equals +0) always by ascending doc id.  A field with "[]" orders a doc by its smallest value when ascending and
        by its largest when descending.  `with_missing=False` lists only docs with a number.  top + skip <= 65536.  On a sharded index the result
        is the shard's part (`partial`): its own first top + skip rows; `merge_top_by` puts the parts of all shards together, no hook is needed."""
        spec = json.dumps({"field": field, "top": top, "skip": skip, "descending": descending, "with_missing": with_missing}).encode()
        h = C.c_void_p()
        _lib.check(self.L.vq_docset_top_by(self.index.h, self._handle(), spec, len(spec), C.byref(h)))
        return TopByResult(self.L, h)

    def timings(self):
        """(mark, count + scan, expand) in ms, recorded when the set was made with VQ_DOCSET_TIMING=1 in the environment; else None"""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        if self.L.vq_debug_docset_timings(self._handle(), C.byref(a), C.byref(b), C.byref(c)) != 0:
            return None
        return a.value, b.value, c.value

    def close(self):
        if getattr(self, "h", None):
            self.L.vq_docset_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TopByResult:
    """The page of `DocSet.top_by` / `merge_top_by` (`vq_docset_top`): numpy arrays `docs` (uint32), `values` (float32: NaN for a NaN doc, 0.0 for a
    missing one), `kinds` (uint8: 0 number, 1 NaN, 2 missing) in row order; `counters`: dict(docs, count, nan, missing) in docs of the set (a
    shard's part: of the set's docs inside the shard); `partial`: a shard's part, to be merged; `pack()`: the flat byte image of the result."""

    def __init__(self, L, h):
        self.L, self.h, self._image = L, h, None
        n = int(L.vq_docset_top_len(h))

        def arr(ptr, dtype):
            return np.frombuffer(C.string_at(ptr, n * np.dtype(dtype).itemsize), dtype=dtype) if n else np.zeros(0, dtype)

        self.docs = arr(L.vq_docset_top_docs(h), np.uint32)
        self.values = arr(L.vq_docset_top_values(h), np.float32)
        self.kinds = arr(L.vq_docset_top_kinds(h), np.uint8)
        c = (C.c_uint64 * 4)()
        L.vq_docset_top_counters(h, c)
        self.counters = {"docs": int(c[0]), "count": int(c[1]), "nan": int(c[2]), "missing": int(c[3])}
        self.partial = bool(L.vq_docset_top_is_partial(h))

    def __len__(self):
        return int(self.docs.size)

    def pack(self):
        """the flat byte image (`vq_docset_top_pack`): what ranks in different processes all-gather; `merge_top_by` takes it as it takes the object"""
        if self._image is None:
            need = int(self.L.vq_docset_top_pack(self.h, None, 0))
            image = C.create_string_buffer(max(need, 1))
            if not need or int(self.L.vq_docset_top_pack(self.h, image, need)) != need:
                raise VelociError(6, self.L.vq_last_error().decode() or "vq_docset_top_pack failed")
            self._image = image.raw[:need]
        return self._image

    def __del__(self):
        if getattr(self, "h", None):
            self.L.vq_docset_top_free(self.h)
            self.h = None

    def rows(self):
        """[(doc, value, kind)]"""
        return list(zip(self.docs.tolist(), self.values.tolist(), self.kinds.tolist()))


def merge_top_by(parts):
    """The parts of one `DocSet.top_by` call on every shard (TopByResult objects or their packed bytes) -> the whole index's page
    (`vq_docset_top_merge`, host only): merged by (sort key, doc), skip and top applied, the counters summed.  Parts whose top, skip, direction,
    with_missing or field differ are refused (VelociError, InvalidArgument), as is a malformed image."""
    L = _lib.lib()
    parts = list(parts)
    own = []  # the handles unpacked here; a result object lends its own
    try:
        handles = []
        for p in parts:
            if isinstance(p, TopByResult):
                handles.append(p.h)
                continue
            image = bytes(p)
            h = C.c_void_p()
            _lib.check(L.vq_docset_top_unpack(image, len(image), C.byref(h)))
            own.append(h)
            handles.append(h)
        out = C.c_void_p()
        _lib.check(L.vq_docset_top_merge((C.c_void_p * max(len(handles), 1))(*handles), len(handles), C.byref(out)))
        return TopByResult(L, out)
    finally:
        for h in own:
            L.vq_docset_top_free(h)


class Request:
    """A parsed search::Request (`vq_request`).  Accepts the reference's JSON (str/bytes) or a dict; `docset`: a DocSet to attach."""

    def __init__(self, request, docset=None):
        if isinstance(request, dict):
            request = json.dumps(request)
        if isinstance(request, str):
            request = request.encode()
        self.L = _lib.lib()
        h = C.c_void_p()
        _lib.check(self.L.vq_request_parse(request, len(request), C.byref(h)))
        self.h = h
        self.has_facets = bool(self.L.vq_request_has_facets(self.h))  # from the PARSED request: decides the exchange path of a sharded step on every rank alike
        if docset is not None:
            self.set_docset(docset)

    def set_docset(self, docset):
        """Attach `docset` (None detaches) — `vq_request_set_docset`.  The request keeps the set alive; its JSON rendering does not change."""
        _lib.check(self.L.vq_request_set_docset(self.h, docset._handle() if docset is not None else None))

    def to_json(self):
        """`vq_request_to_json`: what the parser understood."""
        return self.L.vq_request_to_json(self.h).decode()

    def __del__(self):
        if getattr(self, "h", None):
            self.L.vq_request_free(self.h)
            self.h = None

    def page_after(self, score, doc_id):
        """The continuation of this request behind the ranked hit (score, doc_id) — `vq_request_page_after`."""
        h = C.c_void_p()
        _lib.check(self.L.vq_request_page_after(self.h, C.c_float(float(score)), int(doc_id), C.byref(h)))
        page = Request.__new__(Request)
        page.L, page.h, page.has_facets = self.L, h, False  # (a continuation page carries no facets: page 0 counted them)
        return page

    def top_skip(self):
        """(top, skip) as parsed (top: 10 when absent, search.rs:146)."""
        d = json.loads(self.L.vq_request_to_json(self.h).decode())
        return (10 if d.get("top") is None else int(d["top"])), int(d.get("skip") or 0)


def complete_deep_pages(requests, results, run_page):
    """Requests whose top + skip reaches beyond one scan's ranking come back from the sharded merge as their page 0 (`res.is_page`): page on
    — `run_page(list of Request) -> list of SearchResult` is one more partial -> exchange -> merge round over all shards — and apply skip / top
    (search.rs:230-239).  The host loop of `complete_deep_requests` (exec.cpp) for callers that own the exchange."""
    max_deep, page_len = 65536, 1024
    state = {}
    for i, res in enumerate(results):
        if isinstance(res, SearchResult) and res.is_page:
            req = _as_request(requests[i])
            top, skip = req.top_skip()
            want = top + skip
            res.is_page = False
            ids, scores = res.ids, res.scores
            if skip >= res.num_hits:
                res.ids, res.scores = np.zeros(0, np.uint32), np.zeros(0, np.float32)
                continue
            reach = min(want, res.num_hits)
            if reach > max_deep:
                results[i] = VelociError(4, f"unsupported on the MI355X query path: top + skip reaches more than {max_deep} ranked hits")
                continue
            state[i] = [req, [ids], [scores], len(ids), reach, want, skip]
    pending = sorted(i for i, s in state.items() if s[3] < s[4] and s[3] % page_len == 0 and s[3] > 0)
    while pending:
        pages = [state[i][0].page_after(state[i][2][-1][-1], state[i][1][-1][-1]) for i in pending]
        got = run_page(pages)
        nxt = []
        for i, g in zip(pending, got):
            s = state[i]
            if isinstance(g, VelociError):
                results[i] = g
                state.pop(i)
                continue
            if len(g.ids) == 0:
                continue
            s[1].append(g.ids)
            s[2].append(g.scores)
            s[3] += len(g.ids)
            if s[3] < s[4] and s[3] % page_len == 0:
                nxt.append(i)
        pending = nxt
    for i, s in state.items():
        ids, scores = np.concatenate(s[1]), np.concatenate(s[2])
        results[i].ids, results[i].scores = ids[s[6]:s[5]], scores[s[6]:s[5]]
    return results


def _take_result(L, h):
    try:
        n = L.vq_result_len(h)
        ids = np.ctypeslib.as_array(L.vq_result_ids(h), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        scores = np.ctypeslib.as_array(L.vq_result_scores(h), shape=(n,)).copy() if n else np.zeros(0, np.float32)
        nf = L.vq_result_num_facets(h)
        facets = None
        if nf:
            facets = {}
            for f in range(nf):
                fl = L.vq_result_facet_len(h, f)
                facets[L.vq_result_facet_field(h, f).decode()] = [(L.vq_result_facet_value(h, f, i).decode(), int(L.vq_result_facet_count(h, f, i)))
                                                                   for i in range(fl)]
        res = SearchResult(L.vq_result_num_hits(h), ids, scores, facets, L.vq_result_execution_time_ns(h))
        res.is_page = bool(L.vq_result_is_page(h))  # page 0 of a request that reaches beyond one scan's ranking (sharded merge only)
        wf = L.vq_result_why_found_terms_json(h)  # (requests without why_found / explain: two short strings, no JSON parsing per result)
        res.why_found_terms = {} if wf == b"{}" else json.loads(wf.decode())
        wi = L.vq_result_why_found_info_json(h)  # why_found with select (search.rs:220-224): {anchor id: {field: [highlighted texts]}}; None when not asked
        res.why_found_info = None if wi == b"null" else {int(k): v for k, v in json.loads(wi.decode()).items()}
        ex = L.vq_result_explain_json(h)  # per hit: null or its Explain records (src/search.rs:86,96); "null" without `explain`
        res.explain_json = ex.decode()
        res.explain = None if ex == b"null" else json.loads(res.explain_json)
        return res
    finally:
        L.vq_result_free(h)


def _as_request(r, docset=None):
    """(a Request object handed in with a doc set has the set attached to it, as by set_docset)"""
    if not isinstance(r, Request):
        return Request(r, docset)
    if docset is not None:
        r.set_docset(docset)
    return r


def _with_docsets(requests, docsets):
    if docsets is None:
        return [_as_request(r) for r in requests]
    if len(docsets) != len(requests):
        raise ValueError("docsets: one entry (a DocSet or None) per request")
    return [_as_request(r, d) for r, d in zip(requests, docsets)]


def search(request, index, docset=None):
    """== veloci::search::search(request, &persistence) (src/search.rs:143-228); `docset`: restrict the search to a DocSet's ids."""
    L = _lib.lib()
    req = _as_request(request, docset)
    out = C.c_void_p()
    _lib.check(L.vq_search(index.h, req.h, C.byref(out)))
    return _take_result(L, out)


def suggest(request, index):
    """== search_field::suggest_multi / suggest (src/search/search_field.rs:194-231): `request` is a Request with "suggest" parts or a bare
    RequestSearchPart (dict or JSON).  -> [(text, score, term_id)]"""
    L = _lib.lib()
    if isinstance(request, dict):
        request = json.dumps(request)
    if isinstance(request, str):
        request = request.encode()
    out = C.c_void_p()
    _lib.check(L.vq_suggest_json(index.h, request, len(request), C.byref(out)))
    try:
        return [(L.vq_suggest_text(out, i).decode(), float(L.vq_suggest_score(out, i)), int(L.vq_suggest_term_id(out, i))) for i in range(L.vq_suggest_len(out))]
    finally:
        L.vq_suggest_free(out)


def highlight(part, index):
    """== search_field::highlight (src/search/search_field.rs:233-245): `part` is a RequestSearchPart (dict or JSON) with "snippet": true.
    -> [(snippet, score, text_id)]"""
    L = _lib.lib()
    if isinstance(part, dict):
        part = json.dumps(part)
    if isinstance(part, str):
        part = part.encode()
    out = C.c_void_p()
    _lib.check(L.vq_highlight_json(index.h, part, len(part), C.byref(out)))
    try:
        return [(L.vq_suggest_text(out, i).decode(), float(L.vq_suggest_score(out, i)), int(L.vq_suggest_term_id(out, i))) for i in range(L.vq_suggest_len(out))]
    finally:
        L.vq_suggest_free(out)


def highlight_text(text, terms, snippet_info=None, tokenized=True):
    """== highlight_field::highlight_text (src/highlight_field.rs:92-146) — `vq_highlight_text`.  -> the snippet, or None."""
    L = _lib.lib()
    raw = text.encode()
    enc = [t.encode() for t in terms]
    arr = (C.c_char_p * len(enc))(*enc)
    lens = (C.c_size_t * len(enc))(*[len(e) for e in enc])
    si = json.dumps(snippet_info).encode() if snippet_info is not None else None
    cap = 2 * len(raw) + 256
    while True:
        buf = C.create_string_buffer(cap)
        n = L.vq_highlight_text(raw, len(raw), arr, lens, len(enc), si, len(si) if si else 0, int(tokenized), buf, cap)
        if n == C.c_size_t(-1).value:
            return None
        if n == C.c_size_t(-2).value:
            msg = L.vq_last_error().decode("utf-8", "replace")
            raise _lib.VelociError(1 if msg.startswith("InvalidRequest") else 7 if msg.startswith("JsonError") else 6, msg)
        if n <= cap:
            return buf.raw[:n].decode()
        cap = n


def suggest_batch(requests, index, raise_on_error=True):
    """n independent suggest requests (each as `suggest` takes it) answered as one device batch (`vq_suggest_batch`).
    -> one [(text, score, term_id)] per request; a failing request raises, or with raise_on_error=False yields its VelociError."""
    return _entry_batch(_lib.lib().vq_suggest_batch, requests, index, raise_on_error)


def highlight_batch(parts, index, raise_on_error=True):
    """n independent highlight parts (each as `highlight` takes it) answered as one device batch (`vq_highlight_batch`): the dictionary scans run
    together, a part with `snippet` and its own `top` has its texts ranked and cut to the page on the device and only the page's snippets built.
    -> one [(snippet, score, text_id)] per part; a failing part raises, or with raise_on_error=False yields its VelociError."""
    return _entry_batch(_lib.lib().vq_highlight_batch, parts, index, raise_on_error)


def _entry_batch(entry, requests, index, raise_on_error):
    L = _lib.lib()
    texts = []
    for r in requests:
        if isinstance(r, dict):
            r = json.dumps(r)
        texts.append(r.encode() if isinstance(r, str) else r)
    n = len(texts)
    arr = (C.c_char_p * n)(*texts)
    lens = (C.c_size_t * n)(*[len(t) for t in texts])
    outs = (C.c_void_p * n)()
    status = (C.c_int * n)()
    _lib.check(entry(index.h, arr, lens, n, outs, status))
    first_error = L.vq_last_error().decode("utf-8", "replace")
    results = []
    try:
        for i in range(n):
            if status[i] != 0:
                if raise_on_error:
                    raise VelociError(status[i], first_error)
                results.append(VelociError(status[i], _lib.ERR_NAMES.get(status[i], "error")))
                continue
            out = C.c_void_p(outs[i])
            results.append([(L.vq_suggest_text(out, k).decode(), float(L.vq_suggest_score(out, k)), int(L.vq_suggest_term_id(out, k))) for k in range(L.vq_suggest_len(out))])
    finally:
        for i in range(n):
            if outs[i]:
                L.vq_suggest_free(C.c_void_p(outs[i]))
    return results


def search_batch(requests, index, raise_on_error=True, docsets=None):
    """n independent searches executed as one device batch (`vq_search_batch`); `docsets`: one DocSet or None per request."""
    L = _lib.lib()
    reqs = _with_docsets(requests, docsets)
    n = len(reqs)
    arr = (C.c_void_p * n)(*[r.h for r in reqs])
    outs = (C.c_void_p * n)()
    status = (C.c_int * n)()
    _lib.check(L.vq_search_batch(index.h, arr, n, outs, status))
    results = []
    for i in range(n):
        if status[i] != 0:
            if raise_on_error:
                for j in range(i + 1, n):
                    if outs[j]:
                        L.vq_result_free(C.c_void_p(outs[j]))
                raise VelociError(status[i], L.vq_last_error().decode("utf-8", "replace"))
            results.append(VelociError(status[i], _lib.ERR_NAMES.get(status[i], "error")))
        else:
            results.append(_take_result(L, C.c_void_p(outs[i])))
    return results


COUNTS_NONE = -1  # VQ_COUNTS_NONE: the request needs no count pre-pass


def debug_node_counts(requests, index, summed=True, docsets=None):
    """`vq_debug_node_counts`: what the count pre-pass measures for the requests as one batch, no result scan.  -> one dict per request:
    status (0 counted, COUNTS_NONE, or the error code its search would return), has_filter, filter_count, n_spans, tile_words and
    nodes = [(node id, hits, hits inside the filter)] in counter order.  `summed`: after the sum over the shards (else this shard's numbers)."""
    L = _lib.lib()
    reqs = _with_docsets(requests, docsets)
    n = len(reqs)
    arr = (C.c_void_p * n)(*[r.h for r in reqs])
    cap = 256 * max(n, 1)  # (a count query has at most 127 measured nodes)
    status = np.zeros(n, np.int32)
    has_filter, n_spans, tile_words, node_ids = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(cap, np.uint32)
    filter_count, node_off, hits, inside = np.zeros(n, np.uint64), np.zeros(n + 1, np.uint64), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.vq_debug_node_counts(index.h, arr, n, int(bool(summed)), cap, p(status), p(has_filter), p(filter_count), p(n_spans), p(tile_words), p(node_off),
                                p(node_ids), p(hits), p(inside))
    if rc != 0:
        raise VelociError(5 if rc == -1 else 6, "vq_debug_node_counts: %d (%s)" % (rc, L.vq_last_error().decode("utf-8", "replace")))
    out = []
    for i in range(n):
        lo, hi = int(node_off[i]), int(node_off[i + 1])
        out.append({"status": int(status[i]), "has_filter": bool(has_filter[i]), "filter_count": int(filter_count[i]), "n_spans": int(n_spans[i]),
                    "tile_words": int(tile_words[i]), "nodes": [(int(node_ids[k]), int(hits[k]), int(inside[k])) for k in range(lo, hi)]})
    return out


class RequestBatch:
    """n parsed requests as one C array: build once, search many times (the throughput path)."""

    def __init__(self, requests, docsets=None):
        self.reqs = _with_docsets(requests, docsets)
        self.n = len(self.reqs)
        self.arr = (C.c_void_p * self.n)(*[r.h for r in self.reqs])
        self.has_facets = any(getattr(r, "has_facets", True) for r in self.reqs)
        self._splits = {}

    def split(self, k):
        """k contiguous sub-batches (cached): used to pipeline a large batch."""
        if k <= 1:
            return [self]
        if k not in self._splits:
            self._splits[k] = [RequestBatch(self.reqs[self.n * c // k:self.n * (c + 1) // k]) for c in range(k)]
        return self._splits[k]


def search_batch_flat(batch, index, stride=10, docsets=None):
    """`vq_search_batch_flat`: returns (num_hits u64[n], counts u32[n], ids u32[n, stride], scores f32[n, stride], status i32[n]).
    `docsets`: one DocSet or None per request."""
    L = _lib.lib()
    if not isinstance(batch, RequestBatch):
        batch = RequestBatch(batch, docsets)
    elif docsets is not None:
        _with_docsets(batch.reqs, docsets)
    n = batch.n
    num_hits = np.zeros(n, np.uint64)
    counts = np.zeros(n, np.uint32)
    ids = np.zeros((n, stride), np.uint32)
    scores = np.zeros((n, stride), np.float32)
    status = np.zeros(n, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    _lib.check(L.vq_search_batch_flat(index.h, batch.arr, n, stride, p(num_hits), p(counts), p(ids), p(scores), p(status)))
    return num_hits, counts, ids, scores, status


class PartialBatch:
    """Shard-local partial results of a batch, resident in HBM (`vq_partial_batch`)."""

    def __init__(self, index, requests, slot=None, arena_offset=None):
        """slot / arena_offset: a chunk of a sharded step with one collective (vq_search_batch_partial_at) — its partial is placed at
        `arena_offset` of the index's partial arena instead of its workspace's own buffer."""
        self.L = _lib.lib()
        self.index = index
        self.arena_offset = arena_offset
        self.named = arena_offset is not None  # holds a workspace by name until it is closed (nobody else may take that one meanwhile)
        if isinstance(requests, RequestBatch):
            self.reqs, n, arr = requests.reqs, requests.n, requests.arr
        else:
            self.reqs = [_as_request(r) for r in requests]
            n = len(self.reqs)
            arr = (C.c_void_p * n)(*[r.h for r in self.reqs])
        h = C.c_void_p()
        if arena_offset is None:
            _lib.check(self.L.vq_search_batch_partial(index.h, arr, n, C.byref(h)))
        else:
            _lib.check(self.L.vq_search_batch_partial_at(index.h, arr, n, slot, arena_offset, C.byref(h)))
        self.h = h
        self.n = n

    @property
    def nbytes(self):
        return int(self.L.vq_partial_bytes(self.h))

    @property
    def total_nbytes(self):
        """all-gathered part + histograms: what the partial occupies"""
        return int(self.L.vq_partial_total_bytes(self.h))

    @property
    def device_ptr(self):
        return int(self.L.vq_partial_device_ptr(self.h) or 0)

    @property
    def hist_nbytes(self):
        """Bytes of the batch's facet histograms (u32 counts): summed over the shards by an all-reduce, not gathered."""
        return int(self.L.vq_partial_hist_bytes(self.h))

    @property
    def hist_device_ptr(self):
        return int(self.L.vq_partial_hist_device_ptr(self.h) or 0)

    def merge(self, gathered_device_ptr=None, num_shards=1, raise_on_error=True):
        outs = (C.c_void_p * self.n)()
        status = (C.c_int * self.n)()
        _lib.check(self.L.vq_merge_partials(self.index.h, self.h, C.c_void_p(gathered_device_ptr) if gathered_device_ptr else None, num_shards, outs, status))
        results = []
        for i in range(self.n):
            if status[i] != 0:
                if raise_on_error:
                    raise VelociError(status[i], self.L.vq_last_error().decode("utf-8", "replace"))
                results.append(VelociError(status[i], _lib.ERR_NAMES.get(status[i], "error")))
            else:
                results.append(_take_result(self.L, C.c_void_p(outs[i])))
        return results

    def merge_flat(self, gathered_device_ptr=None, num_shards=1, stride=10, out=None, offset=0, shard_stride=0):
        """out: (num_hits, counts, ids, scores, status) arrays of a larger batch; this partial's rows start at `offset` (a pipeline of
        chunks fills one set of arrays instead of concatenating per-chunk ones)."""
        n = self.n
        if out is None:
            out = (np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros((n, stride), np.uint32), np.zeros((n, stride), np.float32), np.zeros(n, np.int32))
            offset = 0
        num_hits, counts, ids, scores, status = out
        at = lambda a, row: C.c_void_p(a.ctypes.data + row * a.strides[0])
        if shard_stride:  # the shards' copies of this partial lie `shard_stride` bytes apart (one gathered arena holds several partials)
            _lib.check(self.L.vq_merge_partials_flat_strided(self.index.h, self.h, C.c_void_p(gathered_device_ptr), num_shards, shard_stride, stride,
                                                             at(num_hits, offset), at(counts, offset), at(ids, offset), at(scores, offset), at(status, offset)))
            return out
        _lib.check(self.L.vq_merge_partials_flat(self.index.h, self.h, C.c_void_p(gathered_device_ptr) if gathered_device_ptr else None, num_shards, stride,
                                                 at(num_hits, offset), at(counts, offset), at(ids, offset), at(scores, offset), at(status, offset)))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.vq_partial_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
