// Host side of the doc sets (DocSet, engine.hpp): buffers, the launch sequence of docset.hip, the rules of index.cpp for which parts a list carries.
#include <cstdlib>
#include <functional>

#include "engine.hpp"

namespace vq {

// The image from a filled scratch bitmap (engine.hpp)
std::shared_ptr<DocSet> docset_from_marks(const Index& idx, hipStream_t st, uint64_t n, const DocSetMarkFn& mark) {
    static const bool timing = std::getenv("VQ_DOCSET_TIMING") != nullptr;

    auto ds = std::make_shared<DocSet>();
    ds->index_uid = idx.uid;
    ds->num_anchors = idx.num_anchors;
    ds->doc_lo = idx.doc_lo;
    ds->doc_hi = idx.doc_hi;
    ds->device = idx.device;
    ds->stream = st;
    // the image of index.cpp: `words` words from bitmap_base on, one rank entry per 512 docs plus the closing one
    const uint64_t words = idx.bitmap_words, blocks = words >> (kRankShift - 5);
    const uint64_t scratch_words = docset_scratch_words(idx);
    const uint64_t base_word = idx.bitmap_base >> 5;

    DevBuf scratch, local, rank, partials, meta;
    scratch.alloc(scratch_words * 4 + 16);
    local.alloc(words * 4 + 16);
    rank.alloc((blocks + 1) * 4 + 16);
    partials.alloc((blocks / 64u) * 4 + 16);
    meta.alloc(16);
    VQ_HIP(hipMemsetAsync(scratch.p, 0, scratch.bytes, st));
    VQ_HIP(hipMemsetAsync(meta.p, 0, meta.bytes, st));
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EventGuard {
        hipEvent_t* ev;
        ~EventGuard() {
            for (int i = 0; i < 5; ++i)
                if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    } guard{ev};
    if (timing)
        for (auto& e : ev) VQ_HIP(hipEventCreate(&e));
    auto stamp = [&](int i) {
        if (timing) VQ_HIP(hipEventRecord(ev[i], st));
    };
    stamp(0);
    mark(st, scratch.as<uint32_t>(), scratch_words, meta.as<unsigned long long>());
    stamp(1);
    launch_docset_count(st, scratch.as<uint32_t>(), scratch_words, base_word, words, idx.bitmap_base, idx.doc_lo, idx.doc_hi, local.as<uint32_t>(), rank.as<uint32_t>(),
                        meta.as<unsigned long long>());
    launch_docset_scan(st, rank.as<uint32_t>(), blocks, partials.as<uint32_t>());
    stamp(2);
    unsigned long long h_meta[2] = {0, 0};
    uint32_t h_local = 0;
    VQ_HIP(hipMemcpyAsync(h_meta, meta.p, sizeof h_meta, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipMemcpyAsync(&h_local, rank.as<uint32_t>() + blocks, 4, hipMemcpyDeviceToHost, st));
    VQ_HIP(hipStreamSynchronize(st));
    if (h_meta[0])
        throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set: " + std::to_string(h_meta[0]) + " of the " + std::to_string(n) + " ids are not below the index's " +
                                                           std::to_string(idx.num_anchors) + " anchors");
    ds->len = h_meta[1];
    ds->local_len = h_local;

    const uint64_t range = uint64_t(idx.doc_hi) - idx.doc_lo;
    const bool dense = range >= 65536 && uint64_t(h_local) * 64 >= range;   // index.cpp: the lists with a bitmap image
    const bool tiled = range >= 65536 && uint64_t(h_local) * 4096 >= range;  // ... with a tile directory
    ds->docs.alloc(((uint64_t(h_local) + 3u) & ~uint64_t(3)) * 4 + 16);
    stamp(3);
    launch_docset_expand(st, local.as<uint32_t>(), rank.as<uint32_t>(), words, idx.bitmap_base, ds->docs.as<uint32_t>());
    stamp(4);
    if (tiled) {
        ds->tile_entries = (words >> (kTileDirShift - 5)) + 4;  // index.cpp: tiles + 1 entries, tiles = words / 512 + 3
        ds->tile_dir.alloc(ds->tile_entries * 4 + 16);
        launch_docset_tiles(st, rank.as<uint32_t>(), blocks, ds->tile_dir.as<uint32_t>(), ds->tile_entries);
    }
    VQ_HIP(hipStreamSynchronize(st));
    if (timing) {
        VQ_HIP(hipEventElapsedTime(&ds->ms_mark, ev[0], ev[1]));
        VQ_HIP(hipEventElapsedTime(&ds->ms_count_scan, ev[1], ev[2]));
        VQ_HIP(hipEventElapsedTime(&ds->ms_expand, ev[3], ev[4]));
    }
    if (dense) {  // the local slice and its rank directory stay with the set
        ds->bitmap_words = words;
        ds->rank_entries = blocks + 1;
        ds->bitmap = std::move(local);
        ds->rank_dir = std::move(rank);
    }
    ds->device_bytes = ds->docs.bytes + ds->bitmap.bytes + ds->rank_dir.bytes + ds->tile_dir.bytes;
    return ds;
}

std::shared_ptr<const DocSet> make_docset(const Index& idx, const uint32_t* ids, uint64_t n, bool on_device) {
    if (n && !ids) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set: null ids");
    if (on_device && (reinterpret_cast<uintptr_t>(ids) & 3u)) throw VelociError(vqreq::ERR_INVALID_ARGUMENT, "doc set: device ids are not 4-byte aligned");
    VQ_HIP(hipSetDevice(idx.device));
    const hipStream_t st = idx.pre_stream ? idx.pre_stream : idx.stream;
    DevBuf d_ids;
    if (n && !on_device) {
        d_ids.alloc(n * 4 + 16);
        d_ids.upload(ids, n * 4, st);
        ids = d_ids.as<uint32_t>();
    }
    return docset_from_marks(idx, st, n, [&](hipStream_t s, uint32_t* scratch, uint64_t, unsigned long long* meta) { launch_docset_mark(s, ids, n, idx.num_anchors, scratch, meta); });
}

// The set a compiled filter selects (exec.cpp: make_docset_from_filter compiled it and staged `lists` and `fops` on the device).  `st` is the stream
// the compilation's pre-passes ran on.  The scratch bitmap holds the shard's docs only, so its popcount is local: len is the sum over the shards
std::shared_ptr<const DocSet> make_docset_from_program(const Index& idx, hipStream_t st, const DList* lists, uint32_t n_lists, const DOp* fops, uint32_t n_fops,
                                                       uint32_t stack_depth) {
    auto ds = docset_from_marks(idx, st, 0, [&](hipStream_t s, uint32_t* scratch, uint64_t scratch_words, unsigned long long*) {
        launch_docset_filter(s, lists, n_lists, fops, n_fops, stack_depth, idx.doc_lo, idx.doc_hi, scratch, scratch_words);
    });
    if (idx.sharded()) {
        std::vector<uint64_t> total{ds->len};
        idx.sum_over_shards(total);
        ds->len = total[0];
    }
    return ds;
}

}  // namespace vq
