// Host side of the doc set algebra (combine_docsets, engine.hpp): which route fills the scratch bitmap, the launch sequence of docset_algebra.hip in
// rounds of kSetOpTable operands, the sharded length; docset_from_marks (docset.cpp) makes the image from the bits.
#include <algorithm>
#include <cstdlib>

#include "engine.hpp"

namespace vq {

namespace {
SetOperand operand_of(const DocSet& s) { return SetOperand{s.bitmap.as<uint32_t>(), s.docs.as<uint32_t>(), s.local_len, 0u}; }

// round(chunk, count, first) over ops in chunks of kSetOpTable: the table a launch takes is fixed, the number of operands is not
template <class F>
void in_rounds(const SetOperand* ops, size_t n, F&& round) {
    for (size_t at = 0; at < n; at += kSetOpTable) round(ops + at, uint32_t(std::min<size_t>(kSetOpTable, n - at)), at == 0);
}
}  // namespace

std::shared_ptr<const DocSet> combine_docsets(const Index& idx, int op, const std::vector<std::shared_ptr<const DocSet>>& sets) {
    if (op != SETOP_AND && op != SETOP_OR && op != SETOP_MINUS && op != SETOP_NOT) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set algebra: unknown operation " + std::to_string(op));
    if (sets.empty()) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set algebra: no operands");
    if (op == SETOP_NOT && sets.size() != 1) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set algebra: the complement takes one operand, not " + std::to_string(sets.size()));
    for (const auto& s : sets) {
        if (!s) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set algebra: null operand");
        if (s->index_uid != idx.uid) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set algebra: an operand was made for another index");
    }
    if (!idx.can_sum_over_shards())  // the result's length is a sum over the shards
        throw VelociError(vqreq::ERR_UNSUPPORTED, "unsupported on the MI355X query path: doc set algebra on a sharded index without vq_index_set_allreduce");
    VQ_HIP(hipSetDevice(idx.device));
    const hipStream_t st = idx.pre_stream ? idx.pre_stream : idx.stream;

    // The routing rule: the probe route when the result is bounded by a sparse operand — an AND with a bitmap-less operand, a MINUS whose minuend
    // has no bitmap.  VQ_NO_SETOP_PROBE=1 (read at every call) sends everything through the word route.
    const char* no_probe = std::getenv("VQ_NO_SETOP_PROBE");
    const bool probe_allowed = !(no_probe && no_probe[0] && no_probe[0] != '0');
    bool any_sparse = false;
    for (const auto& s : sets) any_sparse = any_sparse || !s->bitmap.p;
    const bool probe = probe_allowed && ((op == SETOP_AND && any_sparse) || (op == SETOP_MINUS && !sets[0]->bitmap.p));

    const uint64_t words = idx.bitmap_words, base_word = idx.bitmap_base >> 5;
    const uint32_t hi = std::min(idx.doc_hi, idx.num_anchors);
    DevBuf temp;  // the word route's AND over a bitmap-less operand: its ids marked into a zeroed bitmap of the scratch bitmap's shape, then folded
    if (!probe && op == SETOP_AND && any_sparse) temp.alloc(docset_scratch_words(idx) * 4 + 16);

    auto ds = docset_from_marks(idx, st, 0, [&](hipStream_t s, uint32_t* scratch, uint64_t scratch_words, unsigned long long* meta) {
        auto fold = [&](const SetOperand* ops, uint32_t n_pos, uint32_t n, bool is_or, bool init_ones) {
            launch_setop_words(s, ops, n_pos, n, is_or, init_ones, scratch, scratch_words, base_word, words, idx.bitmap_base, idx.doc_lo, hi);
        };
        if (probe) {
            size_t lead = 0;  // MINUS: the minuend; AND: the bitmap-less operand with the fewest local ids (the first of them)
            if (op == SETOP_AND) {
                lead = sets.size();
                for (size_t i = 0; i < sets.size(); ++i)
                    if (!sets[i]->bitmap.p && (lead == sets.size() || sets[i]->local_len < sets[lead]->local_len)) lead = i;
            }
            std::vector<SetOperand> others;
            for (size_t i = 0; i < sets.size(); ++i)
                if (i != lead) others.push_back(operand_of(*sets[i]));
            const DocSet& l = *sets[lead];
            if (others.empty()) launch_setop_probe(s, l.docs.as<uint32_t>(), l.local_len, nullptr, 0, op == SETOP_MINUS, false, idx.bitmap_base, scratch);
            in_rounds(others.data(), others.size(), [&](const SetOperand* ops, uint32_t n, bool first) {
                launch_setop_probe(s, l.docs.as<uint32_t>(), l.local_len, ops, n, op == SETOP_MINUS, !first, idx.bitmap_base, scratch);
            });
            return;
        }
        std::vector<SetOperand> with_bitmap, sparse;  // in the caller's order; a MINUS: the subtrahends
        for (size_t i = (op == SETOP_MINUS ? 1 : 0); i < sets.size(); ++i) (sets[i]->bitmap.p ? with_bitmap : sparse).push_back(operand_of(*sets[i]));
        switch (op) {
            case SETOP_OR:  // bitmap-less operands enter by marking
                for (const SetOperand& x : sparse) launch_docset_mark(s, x.docs, x.len, idx.num_anchors, scratch, meta);
                in_rounds(with_bitmap.data(), with_bitmap.size(), [&](const SetOperand* ops, uint32_t n, bool) { fold(ops, 0, n, true, false); });
                break;
            case SETOP_AND: {
                bool first = true;
                in_rounds(with_bitmap.data(), with_bitmap.size(), [&](const SetOperand* ops, uint32_t n, bool) {
                    fold(ops, n, n, false, first);
                    first = false;
                });
                for (const SetOperand& x : sparse) {  // (VQ_NO_SETOP_PROBE only: the rule sends these to the probe route)
                    VQ_HIP(hipMemsetAsync(temp.p, 0, temp.bytes, s));
                    launch_docset_mark(s, x.docs, x.len, idx.num_anchors, temp.as<uint32_t>(), meta);
                    const SetOperand t{temp.as<uint32_t>() + base_word, nullptr, 0u, 0u};  // (the fold reads no word behind the scratch bitmap's end)
                    fold(&t, 1, 1, false, first);
                    first = false;
                }
                break;
            }
            case SETOP_MINUS: {
                bool first = true;
                const SetOperand minuend = operand_of(*sets[0]);
                if (!minuend.bitmap) {  // (VQ_NO_SETOP_PROBE only) the scratch bitmap is the zeroed bitmap its ids are marked into
                    launch_docset_mark(s, minuend.docs, minuend.len, idx.num_anchors, scratch, meta);
                    first = false;
                } else with_bitmap.insert(with_bitmap.begin(), minuend);
                in_rounds(with_bitmap.data(), with_bitmap.size(), [&](const SetOperand* ops, uint32_t n, bool) {
                    fold(ops, first ? 1 : 0, n, false, first);
                    first = false;
                });
                for (const SetOperand& x : sparse) launch_setop_clear(s, x.docs, x.len, scratch);  // bitmap-less subtrahends clear their bits
                break;
            }
            default:  // SETOP_NOT: everything of the doc range, without the operand
                fold(with_bitmap.data(), 0, uint32_t(with_bitmap.size()), false, true);
                for (const SetOperand& x : sparse) launch_setop_clear(s, x.docs, x.len, scratch);
        }
    });
    ds->route = probe ? 1 : 0;
    if (idx.sharded()) {  // the scratch bitmap holds the shard's docs only: its popcount is local
        std::vector<uint64_t> total{ds->len};
        idx.sum_over_shards(total);
        ds->len = total[0];
    }
    return ds;
}

uint64_t copy_docset_ids(const DocSet& ds, uint32_t* out, uint64_t cap, bool on_device) {
    const uint64_t take = std::min<uint64_t>(ds.local_len, cap);
    if (!take) return ds.local_len;
    if (!out) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "vq_docset_ids: null output");
    VQ_HIP(hipSetDevice(ds.device));
    if (on_device) {
        if (reinterpret_cast<uintptr_t>(out) & 3u) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "vq_docset_ids: the device output is not 4-byte aligned");
        VQ_HIP(hipMemcpyAsync(out, ds.docs.p, take * 4, hipMemcpyDeviceToDevice, ds.stream));
        VQ_HIP(hipStreamSynchronize(ds.stream));
    } else VQ_HIP(hipMemcpy(out, ds.docs.p, take * 4, hipMemcpyDeviceToHost));
    return ds.local_len;
}

}  // namespace vq
