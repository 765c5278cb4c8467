// Host side of the numeric aggregations of a doc set (docset_aggregate, engine.hpp): the specs parsed and resolved against the index's columns
// (resolve_range_column: make_docset_from_ranges' own resolution), every edge moved to the f32 grid and turned into an order-preserving key once,
// one state area and one launch per route for all aggregations (docset_aggs.hip: k_docset_agg_ids for the anchor-keyed columns, k_docset_agg_values
// for the 1:n ones), then the download, the sum over the shards with the min / max agreement, and the one rounding of the exact sum.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "engine.hpp"

namespace vq {

namespace {
thread_local float t_last_agg_ms = -1.0f;

uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
float value_of_key(uint32_t key) {  // range_key's inverse (the folded zero comes back as +0.0)
    const uint32_t bits = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
}  // namespace

float docset_aggregate_last_ms() { return t_last_agg_ms; }

double agg_limbs_to_double(const uint64_t* pos, const uint64_t* neg) {
    constexpr int kWords = 12;  // 9 slots of 64 bits at a stride of 32: 8 * 32 + 64 = 320 bits, and one word of room
    auto gather = [](const uint64_t* limb, uint32_t* out) {
        uint64_t carry = 0;
        for (int i = 0; i < kWords; ++i) {
            // slot i contributes its low half here and its high half one word up; both halves and the carry stay below 2^34
            uint64_t t = carry;
            if (i < int(kAggLimbsPerSign)) t += limb[i] & 0xFFFFFFFFull;
            if (i >= 1 && i - 1 < int(kAggLimbsPerSign)) t += limb[i - 1] >> 32;
            out[i] = uint32_t(t);
            carry = t >> 32;
        }
    };
    uint32_t p[kWords], n[kWords], mag[kWords];
    gather(pos, p);
    gather(neg, n);
    int cmp = 0;
    for (int i = kWords - 1; i >= 0 && !cmp; --i) cmp = p[i] != n[i] ? (p[i] > n[i] ? 1 : -1) : 0;
    if (!cmp) return 0.0;
    const uint32_t *big = cmp > 0 ? p : n, *small = cmp > 0 ? n : p;
    uint64_t borrow = 0;
    for (int i = 0; i < kWords; ++i) {
        const uint64_t t = uint64_t(big[i]) - small[i] - borrow;
        mag[i] = uint32_t(t);
        borrow = (t >> 32) & 1u;
    }
    int top = kWords * 32 - 1;  // the highest set bit
    while (!((mag[top >> 5] >> (top & 31)) & 1u)) --top;
    auto bit = [&](int at) { return at >= 0 && ((mag[at >> 5] >> (at & 31)) & 1u); };
    const int shift = top > 52 ? top - 52 : 0;  // bits that do not fit the significand
    uint64_t q = 0;
    for (int at = top; at >= shift; --at) q = (q << 1) | uint64_t(bit(at));
    if (shift) {
        bool sticky = false;
        for (int at = shift - 2; at >= 0 && !sticky; --at) sticky = bit(at);
        if (bit(shift - 1) && (sticky || (q & 1u))) ++q;  // ties to even (q == 2^53 is a double too)
    }
    const double r = std::ldexp(double(q), shift - 149);  // exact: the result lies between 2^-149 and 2^171
    return cmp > 0 ? r : -r;
}

std::vector<AggSpec> agg_specs_from_json(const vqjson::Value& v) {
    if (!v.is_array()) throw vqjson::ParseError("aggregations: expected a sequence", 0);
    if (v.arr.empty()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "aggregations of a doc set: an empty list");
    std::vector<AggSpec> out;
    for (const vqjson::Value& c : v.arr) {
        if (!c.is_object()) throw vqjson::ParseError("aggregation: expected an object", 0);
        for (const auto& m : c.obj)
            if (m.first != "field" && m.first != "edges") throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "aggregations of a doc set: unknown key `" + m.first + "`");
        AggSpec a;
        const vqjson::Value* field = c.get("field");
        if (!field || field->is_null()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "aggregations of a doc set: an aggregation without `field`");
        if (!field->is_string()) throw vqjson::ParseError("aggregation: `field` is not a string", 0);
        a.field = field->str;
        if (const vqjson::Value* e = c.get("edges"); e && !e->is_null()) {
            if (!e->is_array()) throw vqjson::ParseError("aggregation: `edges` is not a sequence", 0);
            a.has_edges = true;
            for (const vqjson::Value& x : e->arr) {
                if (!x.is_number()) throw vqjson::ParseError("aggregation: an edge is not a number", 0);
                a.edges.push_back(x.num);
            }
            if (a.edges.size() > kAggMaxEdges)
                throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "aggregations of a doc set: more than " + std::to_string(kAggMaxEdges) + " edges on " + a.field);
            for (size_t i = 1; i < a.edges.size(); ++i)
                if (!(a.edges[i - 1] < a.edges[i])) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "aggregations of a doc set: the edges on " + a.field + " do not strictly ascend");
        }
        out.push_back(std::move(a));
    }
    return out;
}

std::vector<AggResult> docset_aggregate(const Index& idx, const DocSet& ds, const std::vector<AggSpec>& specs) {
    t_last_agg_ms = -1.0f;
    if (ds.index_uid != idx.uid) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "aggregations of a doc set: the doc set was made for another index");
    if (specs.empty()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "aggregations of a doc set: an empty list");
    if (specs.size() > 65535) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "aggregations of a doc set: more than 65535 aggregations in one call");
    const uint32_t m = uint32_t(specs.size());
    std::vector<RangeColumn> cols;
    cols.reserve(m);
    for (const AggSpec& a : specs) cols.push_back(resolve_range_column(idx, a.field, "aggregations of a doc set"));
    const bool sharded = idx.sharded();
    if (!idx.can_sum_over_shards())  // every number but min and max is a sum over the shards
        throw VelociError(vqreq::ERR_UNSUPPORTED, "unsupported on the MI355X query path: aggregations of a doc set on a sharded index without vq_index_set_allreduce");

    std::vector<AggResult> out(m);
    for (uint32_t i = 0; i < m; ++i) {
        out[i].docs = ds.len;
        out[i].missing = ds.len;
        if (specs[i].has_edges) out[i].buckets.assign(specs[i].edges.size() + 1, 0);
    }
    if (ds.len == 0) return out;  // nothing anywhere: every rank sees len == 0 and none calls the hook

    // the call's device area: [descriptors: the anchor-keyed ones, then the 1:n ones][edge keys][state][min / max keys]
    std::vector<DocsetAggD> descs(m);
    std::vector<uint32_t> order;  // the aggregations in descriptor order
    for (int one_to_n = 0; one_to_n < 2; ++one_to_n)
        for (uint32_t i = 0; i < m; ++i)
            if ((cols[i].to_anchor != nullptr) == (one_to_n != 0)) order.push_back(i);
    uint32_t n_ids = 0, max_keys = 0;
    std::vector<uint32_t> edge_keys, edge_off(m), state_off(m);
    uint64_t state_words = 0;
    for (uint32_t i = 0; i < m; ++i) {
        edge_off[i] = uint32_t(edge_keys.size());
        for (double e : specs[i].edges) edge_keys.push_back(range_key(bits_of(f32_at_or_above(e))));  // (double)v >= e  <=>  key(v) >= this key
        state_off[i] = uint32_t(state_words);
        state_words += kAggBuckets + specs[i].edges.size() + 1;
        if (!cols[i].to_anchor) ++n_ids;
        else max_keys = std::max(max_keys, cols[i].d.num_keys);
    }
    const uint32_t n_vals = m - n_ids;
    const size_t o_desc = 0, o_edges = align_up(o_desc + m * sizeof(DocsetAggD), 256), o_state = align_up(o_edges + edge_keys.size() * 4, 256);
    const size_t o_mm = align_up(o_state + size_t(state_words) * 8, 256), bytes = align_up(o_mm + size_t(m) * 8, 256);

    VQ_HIP(hipSetDevice(idx.device));
    const hipStream_t st = idx.pre_stream ? idx.pre_stream : idx.stream;
    std::vector<uint64_t> state(state_words, 0);
    std::vector<uint32_t> mm(size_t(m) * 2, 0);
    float ms = -1.0f;
    if (ds.local_len) {  // an empty local set launches nothing
        DevBuf area;
        area.alloc(bytes);
        uint8_t* base = area.as<uint8_t>();
        const uint64_t scratch_words = docset_scratch_words(idx);
        std::vector<DevBuf> has_bits(n_vals);
        for (uint32_t k = 0; k < m; ++k) {
            const uint32_t i = order[k];
            DocsetAggD& d = descs[k];
            d = DocsetAggD{};
            d.values = cols[i].d.values;
            d.present = cols[i].d.present;
            d.key_base = cols[i].d.key_base;
            d.num_keys = cols[i].d.num_keys;
            d.edges = reinterpret_cast<const uint32_t*>(base + o_edges) + edge_off[i];
            d.n_edges = uint32_t(specs[i].edges.size());
            d.state_off = state_off[i];
            d.mm_off = 2u * i;
            if (const KVStore* kv = cols[i].to_anchor) {
                d.a_off = kv->d_csr_off.as<uint64_t>();
                d.a_vals = kv->d_text_vals.as<uint32_t>();
                d.a_key_base = kv->key_base;
                d.a_num_keys = kv->num_keys;
                DevBuf& hb = has_bits[k - n_ids];
                hb.alloc(scratch_words * 4 + 16);
                VQ_HIP(hipMemsetAsync(hb.p, 0, hb.bytes, st));
                d.has_bits = hb.as<uint32_t>();
            }
        }
        std::vector<uint8_t> up(bytes, 0);
        std::memcpy(up.data() + o_desc, descs.data(), m * sizeof(DocsetAggD));
        if (!edge_keys.empty()) std::memcpy(up.data() + o_edges, edge_keys.data(), edge_keys.size() * 4);
        for (uint32_t i = 0; i < m; ++i) reinterpret_cast<uint32_t*>(up.data() + o_mm)[2 * i] = 0xFFFFFFFFu;  // the min key; the state and the max key start at zero
        area.upload(up.data(), up.size(), st);

        // VQ_NO_AGG_PREREDUCE=1 (read at every call): every value adds to the sum's limbs with LDS atomics of its own
        const char* no_pre = std::getenv("VQ_NO_AGG_PREREDUCE");
        const bool prereduce = !(no_pre && no_pre[0] && no_pre[0] != '0');
        // VQ_AGG_MAX_GRID=<n> (read at every call): at most n workgroups per aggregation, so that a small set is strided over in many rounds (tests)
        const char* cap = std::getenv("VQ_AGG_MAX_GRID");
        const uint32_t max_grid = cap ? uint32_t(std::strtoul(cap, nullptr, 10)) : 0u;
        static const bool timing = std::getenv("VQ_DOCSET_TIMING") != nullptr;
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
        const DocsetAggD* d_descs = reinterpret_cast<const DocsetAggD*>(base + o_desc);
        unsigned long long* d_state = reinterpret_cast<unsigned long long*>(base + o_state);
        uint32_t* d_mm = reinterpret_cast<uint32_t*>(base + o_mm);
        launch_docset_agg_ids(st, ds.docs.as<uint32_t>(), ds.local_len, d_descs, n_ids, d_state, d_mm, prereduce, max_grid);
        DevBuf scratch, meta;
        if (n_vals) {
            // the membership bitmap: the set's own bitmap image, or (a set without one) its ids marked into a scratch bitmap, as make_docset_from_ranges does
            const uint32_t* member = ds.bitmap.as<uint32_t>();
            uint32_t member_word0 = idx.bitmap_base >> 5;
            if (!member) {
                scratch.alloc(scratch_words * 4 + 16);
                meta.alloc(16);
                VQ_HIP(hipMemsetAsync(scratch.p, 0, scratch.bytes, st));
                VQ_HIP(hipMemsetAsync(meta.p, 0, meta.bytes, st));
                launch_docset_mark(st, ds.docs.as<uint32_t>(), ds.local_len, idx.num_anchors, scratch.as<uint32_t>(), meta.as<unsigned long long>());
                member = scratch.as<uint32_t>();
                member_word0 = 0;
            }
            launch_docset_agg_values(st, d_descs + n_ids, n_vals, max_keys, member, member_word0, idx.doc_lo, std::min(idx.doc_hi, idx.num_anchors), d_state, d_mm, prereduce, max_grid);
        }
        VQ_HIP(hipGetLastError());
        if (timing) VQ_HIP(hipEventRecord(ev[1], st));
        VQ_HIP(hipMemcpyAsync(state.data(), d_state, size_t(state_words) * 8, hipMemcpyDeviceToHost, st));
        VQ_HIP(hipMemcpyAsync(mm.data(), d_mm, size_t(m) * 8, hipMemcpyDeviceToHost, st));
        VQ_HIP(hipStreamSynchronize(st));
        if (timing) VQ_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    }
    t_last_agg_ms = ms;

    // this rank's min / max keys, as far as it counted anything
    std::vector<uint8_t> counted(m);
    for (uint32_t i = 0; i < m; ++i) counted[i] = state[state_off[i] + kAggCount] != 0;
    if (sharded) {
        idx.sum_over_shards(state);  // counters, buckets and limbs: one call
        // min and max cannot be summed: four rounds, one per byte of the key, most significant first.  A rank adds a 1 at its key's digit (256
        // slots for min, 256 for max, per aggregation) while its key's higher bytes equal the prefix agreed so far; the smallest / largest digit
        // anybody named extends the prefix
        std::vector<uint32_t> agreed(size_t(m) * 2, 0);
        std::vector<uint64_t> digits(size_t(m) * 512);
        for (int round = 0; round < 4; ++round) {
            const int low = 24 - 8 * round;
            std::fill(digits.begin(), digits.end(), 0);
            for (uint32_t i = 0; i < m; ++i)
                for (int side = 0; side < 2; ++side) {
                    const uint32_t key = mm[2 * i + side];
                    if (counted[i] && (round == 0 || (key >> (low + 8)) == agreed[2 * i + side])) digits[(size_t(i) * 2 + side) * 256 + ((key >> low) & 0xFFu)] = 1;
                }
            idx.sum_over_shards(digits);
            for (uint32_t i = 0; i < m; ++i)
                for (int side = 0; side < 2; ++side) {
                    const uint64_t* d = digits.data() + (size_t(i) * 2 + side) * 256;
                    uint32_t digit = 0;
                    for (uint32_t k = 0; k < 256; ++k)
                        if (d[k] && (side == 1 || !digit)) {
                            digit = k;
                            if (side == 0) break;
                        }
                    agreed[2 * i + side] = (agreed[2 * i + side] << 8) | digit;
                }
        }
        mm = agreed;
    }

    for (uint32_t i = 0; i < m; ++i) {
        const uint64_t* s = state.data() + state_off[i];
        AggResult& r = out[i];
        r.count = s[kAggCount];
        r.nan = s[kAggNan];
        r.missing = cols[i].to_anchor ? ds.len - s[kAggHas] : s[kAggMissing];
        if (r.count) {
            r.min = value_of_key(mm[2 * i]);
            r.max = value_of_key(mm[2 * i + 1]);
        }
        if (s[kAggPosInf] && s[kAggNegInf]) r.sum = std::numeric_limits<double>::quiet_NaN();
        else if (s[kAggPosInf]) r.sum = std::numeric_limits<double>::infinity();
        else if (s[kAggNegInf]) r.sum = -std::numeric_limits<double>::infinity();
        else r.sum = agg_limbs_to_double(s + kAggLimbs, s + kAggLimbs + kAggLimbsPerSign);
        if (specs[i].has_edges) {
            if (specs[i].edges.empty()) r.buckets[0] = r.count;  // (no edge: the kernels keep no histogram)
            else
                for (size_t b = 0; b < r.buckets.size(); ++b) r.buckets[b] = s[kAggBuckets + b];
        }
    }
    return out;
}

}  // namespace vq
