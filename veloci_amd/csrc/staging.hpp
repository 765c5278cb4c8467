// How the pre-pass runners (prepass.cpp; run_count_queries and run_text_rank in exec.cpp) stage their tables: one device buffer described as
// typed sections, the segmented sorts with their temporary storage, the rows a gather copies, and the two rules every materialised list follows.
#pragma once
#include <algorithm>
#include <cstring>
#include <tuple>
#include <utility>
#include <vector>

#include "engine.hpp"

namespace vq {

// One table of a staged buffer: element type, byte offset, elements, and the arena that laid it out.
template <class T>
struct Section {
    size_t off = 0, n = 0;
    const void* arena = nullptr;
    Section sub(size_t first, size_t count) const {  // elements [first, first + count): what a copy of a part of the table names
        if (first > n || count > n - first) throw VelociError(vqreq::ERR_DEVICE, "internal: a copy beyond its staging section");
        return {off + first * sizeof(T), count, arena};
    }
};

// A device buffer as typed sections, each on a 256-byte boundary.  add() every table, commit() to the buffer (one ensure), then copy and take
// device pointers by handle: the only place where an offset into the buffer becomes a typed pointer.  Handles of another arena are refused.
class StageArena {
    size_t end_ = 0;
    uint8_t* base_ = nullptr;
    bool committed_ = false;

  public:
    template <class T>
    Section<T> add(size_t n) {
        if (committed_) throw VelociError(vqreq::ERR_DEVICE, "internal: a staging section added after commit");
        const Section<T> s{end_, n, this};
        end_ += (n * sizeof(T) + 255) / 256 * 256;
        return s;
    }
    Section<uint8_t> whole() const { return {0, end_, this}; }  // every section as one: a host mirror laid out by the same handles (`mirror + s.off`) goes up in one copy
    void commit(DevBuf& buf, size_t tail = 0) {  // `tail`: slack bytes behind the last section
        buf.ensure(end_ + tail);
        base_ = buf.as<uint8_t>();
        committed_ = true;
    }
    template <class T>
    T* dev(Section<T> s) const {
        if (!committed_ || s.arena != this) throw VelociError(vqreq::ERR_DEVICE, "internal: a staging section used before commit or with another arena");
        return reinterpret_cast<T*>(base_ + s.off);
    }
    template <class T>
    void upload(Section<T> s, const T* src, hipStream_t st) const { if (s.n) VQ_HIP(hipMemcpyAsync(dev(s), src, s.n * sizeof(T), hipMemcpyHostToDevice, st)); }
    template <class T>
    void download(Section<T> s, T* dst, hipStream_t st) const { if (s.n) VQ_HIP(hipMemcpyAsync(dst, dev(s), s.n * sizeof(T), hipMemcpyDeviceToHost, st)); }
    template <class T>
    void zero(Section<T> s, hipStream_t st) const { if (s.n) VQ_HIP(hipMemsetAsync(dev(s), 0, s.n * sizeof(T), st)); }
};

// Entries a materialised list of `len` takes: 8 sentinel entries behind every list, starts stay 16-byte aligned.
inline uint64_t padded_list_len(uint64_t len) { return (len + 8 + 3) / 4 * 4; }

// The largest value of a list from its order-preserving key (device_types.hpp: order_f32).
inline float value_of_order_key(uint32_t key) {
    const uint32_t bits = unorder_f32(key);
    float v;
    std::memcpy(&v, &bits, 4);
    return v;
}

// Segmented radix sort in -> out of u32 or u64 keys: the size query, the temporary storage (kept in `tmp`), the sort.
template <class K>
void seg_sort(DevBuf& tmp, const K* in, K* out, uint32_t n, uint32_t nseg, const uint32_t* seg_begin, const uint32_t* seg_end, hipStream_t st) {
    auto sort = [&](void* storage, size_t bytes) {
        if constexpr (sizeof(K) == 4) return seg_sort_u32(storage, bytes, in, out, n, nseg, seg_begin, seg_end, st);
        else return seg_sort_u64(storage, bytes, in, out, n, nseg, seg_begin, seg_end, st);
    };
    const size_t need = sort(nullptr, 0);
    if (need == size_t(-1)) throw VelociError(vqreq::ERR_DEVICE, "segmented radix sort failed (size query)");
    tmp.ensure(need + 256);
    if (sort(tmp.p, need) == size_t(-1)) throw VelociError(vqreq::ERR_DEVICE, "segmented radix sort failed");
}

// The first half of the text-locality and the 1:n-boost pre-pass: per job, rows of a key-value table gathered into the job's slice of one
// array (k_loc_gather, one launch per table), then every slice sorted.  The jobs come sorted by table.
struct GatherStage {
    std::vector<LocRow> rows;                               // pieces of at most 65536 entries: one workgroup copies one piece
    std::vector<std::pair<size_t, size_t>> table_rows;      // per run of jobs over one table: [first row, end row)
    std::vector<const uint32_t*> table_vals;                // ... and the table's values on the device
    std::vector<uint32_t> seg_begin, seg_end;               // per job: its slice of the gathered array
    uint64_t cursor = 0;                                    // entries gathered so far
    Section<LocRow> s_rows;                                 // where layout() put the rows and the segment bounds
    Section<uint32_t> s_begin, s_end;

    // The next job: the rows of `keys` in `table` (keys outside the table are skipped), cut into pieces.  `overflow`: the caller's message.
    void add_job(const KVStore& table, bool new_table, const std::vector<uint32_t>& keys, const char* overflow) {
        if (new_table) {
            table_rows.push_back({rows.size(), rows.size()});
            table_vals.push_back(table.d_text_vals.as<uint32_t>());
        }
        seg_begin.push_back(uint32_t(cursor));
        for (uint32_t id : keys) {
            if (id < table.key_base || id - table.key_base >= table.num_keys) continue;
            const uint32_t r = id - table.key_base;
            uint64_t src = table.host_off[r], left = table.host_off[r + 1] - table.host_off[r];
            while (left) {
                const uint32_t piece = uint32_t(std::min<uint64_t>(left, 65536));
                rows.push_back(LocRow{src, cursor, piece, 0u});
                src += piece;
                cursor += piece;
                left -= piece;
            }
        }
        if (cursor > 0xFFFFFFF0ull) throw VelociError(vqreq::ERR_UNSUPPORTED, overflow);
        seg_end.push_back(uint32_t(cursor));
        table_rows.back().second = rows.size();
    }
    // After the last job: [rows][seg_begin][seg_end] behind what the caller's arena holds so far; then the three copies up.
    void layout(StageArena& m) { s_rows = m.add<LocRow>(rows.size()); s_begin = m.add<uint32_t>(seg_begin.size()); s_end = m.add<uint32_t>(seg_end.size()); }
    void upload(const StageArena& m, hipStream_t st) const { m.upload(s_rows, rows.data(), st); m.upload(s_begin, seg_begin.data(), st); m.upload(s_end, seg_end.data(), st); }
    // With entries to gather: one gather per table into `a`, sorted into `b`.
    void run(const StageArena& m, DevBuf& a, DevBuf& b, DevBuf& tmp, hipStream_t st) const {
        if (!cursor) return;
        for (size_t t = 0; t < table_rows.size(); ++t)
            launch_loc_gather(st, m.dev(s_rows) + table_rows[t].first, uint32_t(table_rows[t].second - table_rows[t].first), table_vals[t], a.as<uint32_t>());
        VQ_HIP(hipGetLastError());
        seg_sort(tmp, a.as<uint32_t>(), b.as<uint32_t>(), uint32_t(cursor), uint32_t(seg_begin.size()), m.dev(s_begin), m.dev(s_end), st);
    }
};

}  // namespace vq
