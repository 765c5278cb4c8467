// Host side of the doc sets from numeric ranges (make_docset_from_ranges, engine.hpp): the clause list parsed and resolved against the index's
// columns, every bound turned into a closed interval of order-preserving keys (so the kernels compare integers), the route chosen, and the launch
// sequence of docset_ranges.hip in passes of kRangeClauseTable clauses; docset_from_marks (docset.cpp) makes the image from the bits.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"

namespace vq {

namespace {
uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
// the largest f32 (infinities included) that is <= b.  b is no NaN (JSON has none)
float f32_at_or_below(double b) {
    if (b < -double(FLT_MAX)) return -HUGE_VALF;
    if (b > double(FLT_MAX)) return std::isinf(b) ? HUGE_VALF : FLT_MAX;
    float f = float(b);
    if (double(f) > b) f = std::nextafterf(f, -HUGE_VALF);
    return f;
}

}  // namespace

// the smallest f32 (infinities included) that is >= b (engine.hpp: the aggregations' edges use it too)
float f32_at_or_above(double b) {
    if (b > double(FLT_MAX)) return HUGE_VALF;
    if (b < -double(FLT_MAX)) return std::isinf(b) ? -HUGE_VALF : -FLT_MAX;
    float f = float(b);
    if (double(f) < b) f = std::nextafterf(f, HUGE_VALF);
    return f;
}

// the column a clause or an aggregation names, resolved as the request-level boosts resolve it (compile.cpp: anchor-level column boosts)
RangeColumn resolve_range_column(const Index& idx, const std::string& field, const char* what) {
    if (field.find(TOKEN_VALUES) != std::string::npos) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, std::string(what) + ": " + field + " is keyed by term ids, not by docs");
    const auto it = idx.boost.find(field + BOOST_VALID_TO_VALUE);
    if (it == idx.boost.end()) throw VelociError(vqreq::ERR_INDEX_NOT_FOUND, "Did not found path in indices " + field + BOOST_VALID_TO_VALUE);
    RangeColumn col;
    col.d = RangeClauseD{};
    col.d.values = it->second.values.as<uint32_t>();
    col.d.present = it->second.has_present ? it->second.present.as<uint32_t>() : nullptr;
    col.d.key_base = it->second.key_base;
    col.d.num_keys = it->second.num_keys;
    if (field.find("[]") != std::string::npos) {
        const auto kit = idx.kv.find(field + VALUE_ID_TO_ANCHOR);
        if (kit == idx.kv.end() || !kit->second.value_csr) throw VelociError(vqreq::ERR_INDEX_NOT_FOUND, "Did not found path in indices " + field + VALUE_ID_TO_ANCHOR);
        col.to_anchor = &kit->second;
    }
    return col;
}

namespace {
double bound_of(const vqjson::Value& clause, const char* key, bool* has) {
    const vqjson::Value* v = clause.get(key);
    *has = v && !v->is_null();
    if (!*has) return 0.0;
    if (!v->is_number()) throw vqjson::ParseError(std::string("range clause: `") + key + "` is not a number", 0);
    return v->num;
}
}  // namespace

std::vector<RangeClause> range_clauses_from_json(const vqjson::Value& v) {
    if (!v.is_array()) throw vqjson::ParseError("ranges: expected a sequence", 0);
    if (v.arr.empty()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set from ranges: an empty clause list");
    std::vector<RangeClause> out;
    for (const vqjson::Value& c : v.arr) {
        if (!c.is_object()) throw vqjson::ParseError("range clause: expected an object", 0);
        for (const auto& m : c.obj)
            if (m.first != "field" && m.first != "gte" && m.first != "gt" && m.first != "lte" && m.first != "lt" && m.first != "missing")
                throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set from ranges: unknown key `" + m.first + "` in a clause");
        RangeClause rc;
        const vqjson::Value* field = c.get("field");
        if (!field || field->is_null()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set from ranges: a clause without `field`");
        if (!field->is_string()) throw vqjson::ParseError("range clause: `field` is not a string", 0);
        rc.field = field->str;
        bool gte, gt, lte, lt;
        const double b_gte = bound_of(c, "gte", &gte), b_gt = bound_of(c, "gt", &gt), b_lte = bound_of(c, "lte", &lte), b_lt = bound_of(c, "lt", &lt);
        if (gte && gt) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set from ranges: `gt` and `gte` in one clause on " + rc.field);
        if (lte && lt) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set from ranges: `lt` and `lte` in one clause on " + rc.field);
        rc.has_lower = gte || gt;
        rc.lower_open = gt;
        rc.lower = gt ? b_gt : b_gte;
        rc.has_upper = lte || lt;
        rc.upper_open = lt;
        rc.upper = lt ? b_lt : b_lte;
        if (const vqjson::Value* m = c.get("missing"); m && !m->is_null()) {
            if (!m->is_bool()) throw vqjson::ParseError("range clause: `missing` is not a bool", 0);
            rc.missing = m->b;
        }
        out.push_back(std::move(rc));
    }
    return out;
}

// (double)v >= b  <=>  v >= the smallest f32 at or above b, and so on: the bound moves to the f32 grid once, here, and the keys' order is the
// values' (range_key folds -0 onto +0; the slot between key(-denorm_min) and key(0) is empty, so +-1 on a key steps to the neighbouring value)
void range_clause_keys(const RangeClause& c, uint32_t* lo, uint32_t* hi) {
    uint64_t l = kRangeKeyMin, h = kRangeKeyMax;
    if (c.has_lower) {
        const float f = f32_at_or_above(c.lower);
        l = uint64_t(range_key(bits_of(f))) + ((c.lower_open && double(f) == c.lower) ? 1u : 0u);
    }
    if (c.has_upper) {
        const float f = f32_at_or_below(c.upper);
        h = uint64_t(range_key(bits_of(f))) - ((c.upper_open && double(f) == c.upper) ? 1u : 0u);  // (a key is never 0)
    }
    *lo = uint32_t(std::max<uint64_t>(l, kRangeKeyMin));
    *hi = uint32_t(std::min<uint64_t>(h, kRangeKeyMax));
}

std::shared_ptr<const DocSet> make_docset_from_ranges(const Index& idx, const std::vector<RangeClause>& clauses, std::shared_ptr<const DocSet> within) {
    if (clauses.empty()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set from ranges: an empty clause list");
    if (within && within->index_uid != idx.uid) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set from ranges: `within` was made for another index");

    struct OneToN {  // a clause on a field with "[]": its column as the scatter kernel takes it and the table that joins value ids to anchors
        size_t clause;
        RangeClauseD column;
        const KVStore* to_anchor;
    };
    std::vector<RangeClauseD> descs(clauses.size());
    std::vector<OneToN> one_to_n;
    for (size_t i = 0; i < clauses.size(); ++i) {
        const RangeClause& c = clauses[i];
        const RangeColumn col = resolve_range_column(idx, c.field, "doc set from ranges");
        RangeClauseD& d = descs[i];
        d = col.d;
        d.missing = c.missing ? 1u : 0u;
        range_clause_keys(c, &d.lo, &d.hi);
        if (col.to_anchor) one_to_n.push_back(OneToN{i, d, col.to_anchor});
    }
    if (!idx.can_sum_over_shards())  // the result's length is a sum over the shards
        throw VelociError(vqreq::ERR_UNSUPPORTED, "unsupported on the MI355X query path: doc set from ranges on a sharded index without vq_index_set_allreduce");
    VQ_HIP(hipSetDevice(idx.device));
    const hipStream_t st = idx.pre_stream ? idx.pre_stream : idx.stream;

    // The routing rule: the probe route when `within` carries no bitmap (docset_algebra's rule) and every clause is anchor-keyed.
    // VQ_NO_RANGE_PROBE=1 (read at every call) sends everything through the stream route.
    const char* no_probe = std::getenv("VQ_NO_RANGE_PROBE");
    const bool probe_allowed = !(no_probe && no_probe[0] && no_probe[0] != '0');
    const bool probe = probe_allowed && within && !within->bitmap.p && one_to_n.empty();

    const uint32_t hi = std::min(idx.doc_hi, idx.num_anchors);
    const uint64_t clause_words = docset_scratch_words(idx);
    std::vector<DevBuf> clause_bits;  // stream route: per 1:n clause its in-range bitmap, then (missing) its has-a-value bitmap
    if (!probe)
        for (const OneToN& o : one_to_n)
            for (int b = 0; b < (clauses[o.clause].missing ? 2 : 1); ++b) {
                clause_bits.emplace_back();
                clause_bits.back().alloc(clause_words * 4 + 16);
            }

    auto ds = docset_from_marks(idx, st, 0, [&](hipStream_t s, uint32_t* scratch, uint64_t scratch_words, unsigned long long* meta) {
        auto in_passes = [&](auto&& pass) {
            for (size_t at = 0; at < descs.size(); at += kRangeClauseTable) pass(descs.data() + at, uint32_t(std::min<size_t>(kRangeClauseTable, descs.size() - at)), at == 0);
        };
        if (probe) {
            in_passes([&](const RangeClauseD* c, uint32_t n, bool first) { launch_range_probe(s, within->docs.as<uint32_t>(), within->local_len, c, n, !first, scratch); });
            VQ_HIP(hipGetLastError());
            return;
        }
        size_t next = 0;
        for (const OneToN& o : one_to_n) {
            uint32_t* in_bits = clause_bits[next++].as<uint32_t>();
            uint32_t* has_bits = clauses[o.clause].missing ? clause_bits[next++].as<uint32_t>() : nullptr;
            VQ_HIP(hipMemsetAsync(in_bits, 0, clause_words * 4, s));
            if (has_bits) VQ_HIP(hipMemsetAsync(has_bits, 0, clause_words * 4, s));
            const KVStore& kv = *o.to_anchor;
            launch_range_scatter(s, o.column, kv.d_csr_off.as<uint64_t>(), kv.d_text_vals.as<uint32_t>(), kv.key_base, kv.num_keys, idx.doc_lo, hi, in_bits, has_bits);
            RangeClauseD& d = descs[o.clause];
            d.values = in_bits;
            d.present = has_bits;
            d.bitmap = 1u;
        }
        // `within` enters as the first pass's mask: its bitmap image, or (a set without one: a 1:n clause or VQ_NO_RANGE_PROBE brought it here) its ids
        // marked into the scratch bitmap, which every pass then and-s into
        const uint32_t* mask = nullptr;
        uint32_t mask_word0 = 0;
        if (within && within->bitmap.p) {
            mask = within->bitmap.as<uint32_t>();
            mask_word0 = idx.bitmap_base >> 5;
        } else if (within) {
            launch_docset_mark(s, within->docs.as<uint32_t>(), within->local_len, idx.num_anchors, scratch, meta);
            mask = scratch;
        }
        in_passes([&](const RangeClauseD* c, uint32_t n, bool first) {
            launch_range_bits(s, c, n, first ? mask : scratch, first ? mask_word0 : 0u, scratch, scratch_words, idx.doc_lo, hi);
        });
        VQ_HIP(hipGetLastError());
    });
    ds->range_route = probe ? 1 : 0;
    if (idx.sharded()) {  // the scratch bitmap holds the shard's docs only: its popcount is local
        std::vector<uint64_t> total{ds->len};
        idx.sum_over_shards(total);
        ds->len = total[0];
    }
    return ds;
}

}  // namespace vq
