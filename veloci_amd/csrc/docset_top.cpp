// Host side of a doc set ordered by a column (docset_top, engine.hpp): the spec parsed and its column resolved (resolve_range_column: the
// resolution of make_docset_from_ranges and docset_aggregate), one scratch area and the kernel sequence of docset_top.hip on one stream, the
// download of at most top + skip (sort key, doc) pairs, their final order, and the host-only protocol of shard parts: merge, pack, unpack.
//
// The final order of the at most kTopMaxRows pairs is made here, on the host, after the download (top_sort_pairs).  Measured on the bench index
// (profiles/docset_top/README.md): a page of 10 pairs costs 0.014 ms downloaded and sorted on the host against 0.029 ms sorted by a device radix
// sort and then downloaded; a page of 65 536 pairs 0.21 ms against 0.11 ms.  The host order wins where calls are frequent and loses a tenth of a
// millisecond at the largest page, and it needs no temporary area and no further launches.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "engine.hpp"

namespace vq {

namespace {
thread_local float t_last_top_ms = -1.0f;

float top_value_of_key(uint32_t key) {  // range_key's inverse (the folded zero comes back as +0.0)
    const uint32_t bits = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
// docs / keys -> values and kinds
void top_fill_rows(TopResult& r) {
    const size_t n = r.keys.size();
    r.values.resize(n);
    r.kinds.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t key = r.keys[i];
        if (key == kTopMissingKey) {
            r.kinds[i] = 2;
            r.values[i] = 0.0f;
        } else if (key == kTopNanKey) {
            r.kinds[i] = 1;
            r.values[i] = std::numeric_limits<float>::quiet_NaN();
        } else {
            r.kinds[i] = 0;
            r.values[i] = top_value_of_key(r.spec.descending ? ~key : key);
        }
    }
}
// sorted (key << 32 | doc) pairs, cut to the numbers unless with_missing, rows [skip, skip + top) -> the result's rows
void top_take_rows(TopResult& r, std::vector<uint64_t>& pairs, uint64_t skip, uint64_t top) {
    if (!r.spec.with_missing)
        while (!pairs.empty() && uint32_t(pairs.back() >> 32) > kRangeKeyMax) pairs.pop_back();
    const size_t lo = size_t(std::min<uint64_t>(skip, pairs.size())), hi = size_t(std::min<uint64_t>(skip + top, pairs.size()));
    r.docs.clear();
    r.keys.clear();
    for (size_t i = lo; i < hi; ++i) {
        r.keys.push_back(uint32_t(pairs[i] >> 32));
        r.docs.push_back(uint32_t(pairs[i]));
    }
    top_fill_rows(r);
}
uint32_t top_u32(const vqjson::Value& v, const char* name) {
    if (!v.is_number()) throw vqjson::ParseError(std::string("top_by: `") + name + "` is not a number", 0);
    if (!(v.num >= 0.0) || v.num > 4294967295.0 || v.num != std::floor(v.num))
        throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string("a doc set ordered by a column: `") + name + "` is no unsigned 32-bit integer");
    return uint32_t(v.num);
}
// ascending order of (key << 32 | doc) pairs: a byte-wise radix sort that skips the bytes all pairs share (a page's keys often share their top
// bytes, its docs never all eight), std::sort for short pages
void top_sort_pairs(std::vector<uint64_t>& pairs) {
    const size_t n = pairs.size();
    if (n < 2048) {
        std::sort(pairs.begin(), pairs.end());
        return;
    }
    uint64_t all_or = 0, all_and = ~uint64_t(0);
    for (uint64_t p : pairs) {
        all_or |= p;
        all_and &= p;
    }
    const uint64_t varies = all_or ^ all_and;
    std::vector<uint64_t> tmp(n);
    uint64_t *from = pairs.data(), *to = tmp.data();
    for (int shift = 0; shift < 64; shift += 8) {
        if (!((varies >> shift) & 0xFFu)) continue;
        size_t count[257] = {0};
        for (size_t i = 0; i < n; ++i) ++count[((from[i] >> shift) & 0xFFu) + 1u];
        for (int b = 0; b < 256; ++b) count[b + 1] += count[b];
        for (size_t i = 0; i < n; ++i) to[count[(from[i] >> shift) & 0xFFu]++] = from[i];
        std::swap(from, to);
    }
    if (from != pairs.data()) pairs.swap(tmp);
}
bool top_env_flag(const char* name) {
    const char* v = std::getenv(name);
    return v && v[0] && v[0] != '0';
}

// the byte image of a result: kTopImageHeader bytes, the field padded to a multiple of 8 bytes, then rows x (sort key u32, doc u32)
constexpr uint32_t kTopImageMagic = 0x50545156u, kTopImageVersion = 1u;  // "VQTP"
constexpr size_t kTopImageHeader = 64, kTopMaxField = 4096;
struct TopImageHeader {
    uint32_t magic, version, flags, top, skip, rows, field_len, pad;  // flags: 1 descending, 2 with_missing, 4 partial
    uint64_t n_docs, count, nan, missing;
};
static_assert(sizeof(TopImageHeader) == kTopImageHeader, "the image header is a fixed 64 bytes");
}  // namespace

float docset_top_last_ms() { return t_last_top_ms; }

TopSpec top_spec_from_json(const vqjson::Value& v) {
    if (!v.is_object()) throw vqjson::ParseError("top_by: expected an object", 0);
    for (const auto& m : v.obj)
        if (m.first != "field" && m.first != "top" && m.first != "skip" && m.first != "descending" && m.first != "with_missing")
            throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "a doc set ordered by a column: unknown key `" + m.first + "`");
    TopSpec s;
    const vqjson::Value* field = v.get("field");
    if (!field || field->is_null()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "a doc set ordered by a column: a spec without `field`");
    if (!field->is_string()) throw vqjson::ParseError("top_by: `field` is not a string", 0);
    s.field = field->str;
    if (const vqjson::Value* x = v.get("top"); x && !x->is_null()) s.top = top_u32(*x, "top");
    if (const vqjson::Value* x = v.get("skip"); x && !x->is_null()) s.skip = top_u32(*x, "skip");
    if (const vqjson::Value* x = v.get("descending"); x && !x->is_null()) {
        if (!x->is_bool()) throw vqjson::ParseError("top_by: `descending` is not a boolean", 0);
        s.descending = x->b;
    }
    if (const vqjson::Value* x = v.get("with_missing"); x && !x->is_null()) {
        if (!x->is_bool()) throw vqjson::ParseError("top_by: `with_missing` is not a boolean", 0);
        s.with_missing = x->b;
    }
    return s;
}

TopResult docset_top(const Index& idx, const DocSet& ds, const TopSpec& spec) {
    t_last_top_ms = -1.0f;
    const char* what = "a doc set ordered by a column";
    if (ds.index_uid != idx.uid) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": the doc set was made for another index");
    const RangeColumn col = resolve_range_column(idx, spec.field, what);
    if (uint64_t(spec.top) + spec.skip > kTopMaxRows)
        throw VelociError(vqreq::ERR_UNSUPPORTED, "unsupported on the MI355X query path: a doc set ordered by a column with top + skip above " + std::to_string(kTopMaxRows) +
                                                      " (the search's bound on ranked hits)");
    TopResult r;
    r.spec = spec;
    r.partial = idx.sharded();
    const uint32_t n = ds.local_len, rows = spec.top + spec.skip;
    r.n_docs = n;
    if (!n) return r;  // an empty local set launches nothing

    // the call's device area: [state][4 histograms][chunk counts][keys][out pairs]
    const uint32_t cap = std::min(rows, n);
    const size_t n_pad = (size_t(n) + 3u) & ~size_t(3);
    const size_t o_state = 0, o_hist = o_state + kTopStateWords * 4, o_chunks = o_hist + 4 * 256 * 4, o_keys = align_up(o_chunks + kTopMaxGrid * 4, 256);
    const size_t o_out = align_up(o_keys + n_pad * 4, 256), bytes = align_up(o_out + size_t(cap) * 8 + 8, 256);
    const size_t head = o_keys;  // what is zeroed (or preset) before the launches

    VQ_HIP(hipSetDevice(idx.device));
    const hipStream_t st = idx.pre_stream ? idx.pre_stream : idx.stream;
    // VQ_TOP_MAX_GRID=<n> (read at every call): at most n workgroups per kernel, so that a small set runs in many strided rounds and tie chunks (tests)
    const char* grid_cap = std::getenv("VQ_TOP_MAX_GRID");
    const uint32_t max_grid = grid_cap ? uint32_t(std::strtoul(grid_cap, nullptr, 10)) : 0u;
    // VQ_TOP_FORCE_SELECT=1 (read at every call): the select runs even when every local id is a winner (tests)
    const bool select = n > rows || top_env_flag("VQ_TOP_FORCE_SELECT");
    static const bool timing = std::getenv("VQ_DOCSET_TIMING") != nullptr;

    DevBuf area;
    area.alloc(bytes);
    uint8_t* base = area.as<uint8_t>();
    uint32_t* d_state = reinterpret_cast<uint32_t*>(base + o_state);
    uint32_t* d_hist = reinterpret_cast<uint32_t*>(base + o_hist);
    uint32_t* d_chunks = reinterpret_cast<uint32_t*>(base + o_chunks);
    uint32_t* d_keys = reinterpret_cast<uint32_t*>(base + o_keys);
    unsigned long long* d_out = reinterpret_cast<unsigned long long*>(base + o_out);
    std::vector<uint32_t> up(head / 4, 0);
    if (!select) {  // every local id is a winner: the emit takes every key through the cursor
        up[kTopT] = kTopMissingKey;
        up[kTopAllTies] = 1u;
    }
    area.upload(up.data(), head, st);

    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EventGuard {
        hipEvent_t* ev;
        ~EventGuard() {
            for (int i = 0; i < 2; ++i)
                if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    } guard{ev};
    if (timing) {
        for (auto& e : ev) VQ_HIP(hipEventCreate(&e));
        VQ_HIP(hipEventRecord(ev[0], st));
    }
    DocsetTopD d{};
    d.values = col.d.values;
    d.present = col.d.present;
    d.key_base = col.d.key_base;
    d.num_keys = col.d.num_keys;
    d.doc_lo = idx.doc_lo;
    d.descending = spec.descending ? 1u : 0u;
    DevBuf best, scratch, meta;
    if (const KVStore* kv = col.to_anchor) {
        d.a_off = kv->d_csr_off.as<uint64_t>();
        d.a_vals = kv->d_text_vals.as<uint32_t>();
        d.a_key_base = kv->key_base;
        d.a_num_keys = kv->num_keys;
        const uint32_t doc_hi = std::min(idx.doc_hi, idx.num_anchors);
        best.alloc(size_t(doc_hi - idx.doc_lo) * 4 + 16);  // 4 B per doc of the index's doc range
        VQ_HIP(hipMemsetAsync(best.p, 0xFF, best.bytes, st));
        // the membership bitmap: the set's own bitmap image, or (a set without one) its ids marked into a scratch bitmap, as docset_aggregate does
        const uint32_t* member = ds.bitmap.as<uint32_t>();
        uint32_t member_word0 = idx.bitmap_base >> 5;
        if (!member) {
            const uint64_t scratch_words = docset_scratch_words(idx);
            scratch.alloc(scratch_words * 4 + 16);
            meta.alloc(16);
            VQ_HIP(hipMemsetAsync(scratch.p, 0, scratch.bytes, st));
            VQ_HIP(hipMemsetAsync(meta.p, 0, meta.bytes, st));
            launch_docset_mark(st, ds.docs.as<uint32_t>(), n, idx.num_anchors, scratch.as<uint32_t>(), meta.as<unsigned long long>());
            member = scratch.as<uint32_t>();
            member_word0 = 0;
        }
        launch_top_fold(st, d, member, member_word0, doc_hi, best.as<uint32_t>(), max_grid);
        d.best = best.as<uint32_t>();
    }
    const uint32_t* d_docs = ds.docs.as<uint32_t>();
    launch_top_keys(st, d_docs, n, d, d_keys, d_hist, d_state, max_grid);
    if (select) {
        for (uint32_t pass = 0; pass < 4; ++pass) {
            const uint32_t shift = 24u - 8u * pass;
            if (pass) launch_top_hist(st, d_keys, n, shift, d_state, d_hist + 256u * pass, max_grid);
            launch_top_pick(st, d_state, d_hist + 256u * pass, shift, rows, spec.with_missing, n);
        }
        launch_top_tiecount(st, d_keys, n, d_state, d_chunks, max_grid);
    }
    launch_top_emit(st, d_docs, d_keys, n, d_state, d_chunks, d_out, cap, max_grid);
    VQ_HIP(hipGetLastError());
    if (timing) VQ_HIP(hipEventRecord(ev[1], st));
    std::vector<uint32_t> state(kTopStateWords, 0);
    std::vector<uint64_t> pairs(cap, 0);
    VQ_HIP(hipMemcpyAsync(state.data(), d_state, kTopStateWords * 4, hipMemcpyDeviceToHost, st));
    if (cap) VQ_HIP(hipMemcpyAsync(pairs.data(), d_out, size_t(cap) * 8, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    float ms = -1.0f;
    if (timing) VQ_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    t_last_top_ms = ms;

    r.count = state[kTopCount];
    r.nan = state[kTopNan];
    r.missing = state[kTopMissing];
    if (r.count + r.nan + r.missing != n) throw VelociError(vqreq::ERR_DEVICE, std::string(what) + ": the counters do not add up to the set");
    const uint64_t eligible = spec.with_missing ? n : r.count;
    const uint64_t emitted = select ? std::min<uint64_t>(rows, eligible) : n;  // (without select every key came back: cap == n)
    if (emitted > cap || state[kTopCursor] > cap) throw VelociError(vqreq::ERR_DEVICE, std::string(what) + ": more rows than the page holds");
    pairs.resize(size_t(emitted));
    top_sort_pairs(pairs);
    for (size_t i = 1; i < pairs.size(); ++i)
        if (pairs[i - 1] == pairs[i]) throw VelociError(vqreq::ERR_DEVICE, std::string(what) + ": a row came back twice");
    top_take_rows(r, pairs, r.partial ? 0 : spec.skip, r.partial ? rows : spec.top);  // a shard's part keeps its first top + skip rows
    return r;
}

TopResult docset_top_merge(const std::vector<const TopResult*>& parts) {
    const char* what = "merge of doc sets ordered by a column";
    if (parts.empty()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": no part");
    for (const TopResult* p : parts)
        if (!p) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": a part is null");
    const TopSpec& s = parts[0]->spec;
    for (const TopResult* p : parts) {
        if (p->spec.top != s.top) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": the parts differ in `top`");
        if (p->spec.skip != s.skip) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": the parts differ in `skip`");
        if (p->spec.descending != s.descending) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": the parts differ in `descending`");
        if (p->spec.with_missing != s.with_missing) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": the parts differ in `with_missing`");
        if (p->spec.field != s.field) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": the parts differ in `field`");
        if (!p->partial && parts.size() > 1) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": a whole index's result among the parts");
        if (p->docs.size() != p->keys.size()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": a part whose rows are incomplete");
    }
    TopResult r;
    r.spec = s;
    r.partial = false;
    if (!parts[0]->partial) {  // one whole result: skip and top are applied already
        r = *parts[0];
        return r;
    }
    std::vector<uint64_t> pairs;
    for (const TopResult* p : parts) {
        r.n_docs += p->n_docs;
        r.count += p->count;
        r.nan += p->nan;
        r.missing += p->missing;
        for (size_t i = 0; i < p->docs.size(); ++i) pairs.push_back((uint64_t(p->keys[i]) << 32) | p->docs[i]);
    }
    top_sort_pairs(pairs);  // every part holds its own first top + skip rows: the whole index's first top + skip are among them
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    top_take_rows(r, pairs, s.skip, s.top);
    return r;
}

std::vector<uint8_t> docset_top_pack(const TopResult& r) {
    if (r.spec.field.size() > kTopMaxField) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "pack of a doc set ordered by a column: a field name of more than 4096 bytes");
    if (r.docs.size() != r.keys.size() || r.docs.size() > kTopMaxRows) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "pack of a doc set ordered by a column: rows that are incomplete");
    TopImageHeader h{};
    h.magic = kTopImageMagic;
    h.version = kTopImageVersion;
    h.flags = (r.spec.descending ? 1u : 0u) | (r.spec.with_missing ? 2u : 0u) | (r.partial ? 4u : 0u);
    h.top = r.spec.top;
    h.skip = r.spec.skip;
    h.rows = uint32_t(r.docs.size());
    h.field_len = uint32_t(r.spec.field.size());
    h.n_docs = r.n_docs;
    h.count = r.count;
    h.nan = r.nan;
    h.missing = r.missing;
    const size_t field_room = align_up(r.spec.field.size(), 8);
    std::vector<uint8_t> out(kTopImageHeader + field_room + r.docs.size() * 8, 0);
    std::memcpy(out.data(), &h, sizeof h);
    if (!r.spec.field.empty()) std::memcpy(out.data() + kTopImageHeader, r.spec.field.data(), r.spec.field.size());
    uint8_t* rows = out.data() + kTopImageHeader + field_room;
    for (size_t i = 0; i < r.docs.size(); ++i) {
        std::memcpy(rows + 8 * i, &r.keys[i], 4);
        std::memcpy(rows + 8 * i + 4, &r.docs[i], 4);
    }
    return out;
}

TopResult docset_top_unpack(const uint8_t* bytes, size_t len) {
    auto bad = [](const char* why) { return VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string("unpack of a doc set ordered by a column: ") + why); };
    if (!bytes || len < kTopImageHeader) throw bad("an image shorter than its header");
    TopImageHeader h;
    std::memcpy(&h, bytes, sizeof h);
    if (h.magic != kTopImageMagic || h.version != kTopImageVersion) throw bad("not an image of this version");
    if ((h.flags & ~7u) || h.pad) throw bad("unknown flags");
    if (uint64_t(h.top) + h.skip > kTopMaxRows) throw bad("top + skip above the bound");
    const bool partial = (h.flags & 4u) != 0;
    if (h.rows > (partial ? h.top + h.skip : h.top)) throw bad("more rows than the page holds");
    if (h.field_len > kTopMaxField) throw bad("a field name of more than 4096 bytes");
    const size_t field_room = align_up(size_t(h.field_len), 8);
    if (len != kTopImageHeader + field_room + size_t(h.rows) * 8) throw bad("the length does not match the header");
    if (h.count > h.n_docs || h.nan > h.n_docs || h.missing > h.n_docs || h.count + h.nan + h.missing != h.n_docs) throw bad("counters that do not add up");
    if (h.rows > h.n_docs) throw bad("more rows than docs");
    for (size_t i = h.field_len; i < field_room; ++i)
        if (bytes[kTopImageHeader + i]) throw bad("padding that is not zero");
    TopResult r;
    r.spec.field.assign(reinterpret_cast<const char*>(bytes) + kTopImageHeader, h.field_len);
    r.spec.top = h.top;
    r.spec.skip = h.skip;
    r.spec.descending = (h.flags & 1u) != 0;
    r.spec.with_missing = (h.flags & 2u) != 0;
    r.partial = partial;
    r.n_docs = h.n_docs;
    r.count = h.count;
    r.nan = h.nan;
    r.missing = h.missing;
    const uint8_t* rows = bytes + kTopImageHeader + field_room;
    r.keys.resize(h.rows);
    r.docs.resize(h.rows);
    for (size_t i = 0; i < h.rows; ++i) {
        std::memcpy(&r.keys[i], rows + 8 * i, 4);
        std::memcpy(&r.docs[i], rows + 8 * i + 4, 4);
        const uint32_t key = r.keys[i];
        if (key < kRangeKeyMin || (key > kRangeKeyMax && key < kTopNanKey)) throw bad("a sort key that no value has");
        if (!r.spec.with_missing && key > kRangeKeyMax) throw bad("a row without a number in a page of numbers");
        if (i && ((uint64_t(r.keys[i - 1]) << 32) | r.docs[i - 1]) >= ((uint64_t(key) << 32) | r.docs[i])) throw bad("rows that do not ascend");
    }
    top_fill_rows(r);
    return r;
}

}  // namespace vq
