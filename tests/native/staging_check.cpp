// TEST INFRASTRUCTURE — the staging helpers of the pre-pass runners (veloci_amd/csrc/staging.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer,
// as a program of its own (run by tests/test_prepass_staging_cpu.py) over the stubbed device layer, where "device" memory is host memory:
// StageArena (section starts, overlaps, committed size, copies and their sub-ranges, zero, empty sections, add after commit), the row cutter of
// GatherStage against a plain loop (it stops before the launches, which throw in the stub), padded_list_len.  Prints STAGING_CHECK_OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../veloci_amd/csrc/staging.hpp"

extern "C" long vq_stub_async_calls();

#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

using namespace vq;

namespace {
struct B24 {
    uint64_t a, b, c;
};
static_assert(sizeof(B24) == 24, "a 24-byte element");
const size_t kCounts[5] = {0, 1, 255, 256, 257};
long g_sections = 0, g_arenas = 0;

struct Extent {  // what the checks below need of a section, whatever its element type
    size_t off, bytes;
};

// One section of `n` elements of T in a committed arena: round trips and zero stay inside it.
template <class T>
void check_section(const StageArena& a, Section<T> s, uint8_t* base, size_t total, hipStream_t st) {
    ++g_sections;
    const size_t bytes = s.n * sizeof(T);
    std::vector<uint8_t> before(base, base + total);
    const long calls = vq_stub_async_calls();
    std::vector<T> up(s.n), down(s.n);
    if (bytes) std::memset(static_cast<void*>(up.data()), 0x5A, bytes);
    a.upload(s, up.data(), st);
    a.download(s, down.data(), st);
    CHECK(vq_stub_async_calls() - calls == (s.n ? 2 : 0));  // an empty section issues no copy
    CHECK(bytes == 0 || std::memcmp(up.data(), down.data(), bytes) == 0);
    CHECK(reinterpret_cast<uint8_t*>(a.dev(s)) == base + s.off);
    if (s.n >= 3) {  // "the first n" and "from element k": elements [1, n - 1) only
        std::vector<T> mid(s.n - 2), got(s.n - 2), first(2);
        std::memset(static_cast<void*>(mid.data()), 0xC3, mid.size() * sizeof(T));
        a.upload(s.sub(1, mid.size()), mid.data(), st);
        a.download(s.sub(1, got.size()), got.data(), st);
        CHECK(std::memcmp(mid.data(), got.data(), mid.size() * sizeof(T)) == 0);
        a.download(s.sub(0, 2), first.data(), st);
        CHECK(std::memcmp(&first[0], &up[0], sizeof(T)) == 0 && std::memcmp(&first[1], &mid[0], sizeof(T)) == 0);
        a.download(s.sub(s.n - 1, 1), first.data(), st);  // from element n - 1 to the end: one element
        CHECK(std::memcmp(&first[0], &up[s.n - 1], sizeof(T)) == 0);
        bool threw = false;
        try {
            a.download(s.sub(1, s.n), got.data(), st);  // one past the section
        } catch (const VelociError&) {
            threw = true;
        }
        CHECK(threw);
        threw = false;
        try {
            StageArena other;
            other.add<T>(s.n);
            DevBuf other_buf;
            other.commit(other_buf);
            other.download(s, got.data(), st);  // a handle of another arena
        } catch (const VelociError&) {
            threw = true;
        }
        CHECK(threw);
    }
    // everything outside the section is as it was; zero clears exactly the section
    CHECK(std::memcmp(base, before.data(), s.off) == 0 && std::memcmp(base + s.off + bytes, before.data() + s.off + bytes, total - s.off - bytes) == 0);
    const long zcalls = vq_stub_async_calls();
    a.zero(s, st);
    CHECK(vq_stub_async_calls() - zcalls == (s.n ? 1 : 0));
    for (size_t i = 0; i < bytes; ++i) CHECK(base[s.off + i] == 0);
    CHECK(std::memcmp(base, before.data(), s.off) == 0 && std::memcmp(base + s.off + bytes, before.data() + s.off + bytes, total - s.off - bytes) == 0);
    std::memcpy(base + s.off, before.data() + s.off, bytes);  // (the pattern again, for the next section's neighbours)
}

// Sections of the five counts in the order `order`, element sizes rotating from `rot`; `tail` bytes behind the last one.
void check_arena(const int (&order)[5], int rot, size_t tail) {
    ++g_arenas;
    StageArena a;
    Section<uint8_t> s1[5];
    Section<uint32_t> s4[5];
    Section<uint64_t> s8[5];
    Section<B24> s24[5];
    std::vector<Extent> ext;
    for (int k = 0; k < 5; ++k) {
        const size_t n = kCounts[order[k]];
        switch ((k + rot) % 4) {
            case 0: s1[k] = a.add<uint8_t>(n); ext.push_back({s1[k].off, n}); break;
            case 1: s4[k] = a.add<uint32_t>(n); ext.push_back({s4[k].off, n * 4}); break;
            case 2: s8[k] = a.add<uint64_t>(n); ext.push_back({s8[k].off, n * 8}); break;
            default: s24[k] = a.add<B24>(n); ext.push_back({s24[k].off, n * 24}); break;
        }
    }
    for (size_t i = 0; i < ext.size(); ++i) {
        CHECK(ext[i].off % 256 == 0);
        for (size_t j = 0; j < i; ++j) CHECK(ext[j].off + ext[j].bytes <= ext[i].off);  // (added in ascending order: no overlap)
    }
    DevBuf buf;
    a.commit(buf, tail);
    CHECK(buf.bytes >= ext.back().off + ext.back().bytes + tail && a.whole().n >= ext.back().off + ext.back().bytes && a.whole().off == 0);
    bool threw = false;
    try {
        a.add<uint32_t>(1);
    } catch (const VelociError& e) {
        threw = e.code == vqreq::ERR_DEVICE;
    }
    CHECK(threw);
    uint8_t* base = buf.as<uint8_t>();
    const size_t total = ext.back().off + ext.back().bytes + tail;
    for (size_t i = 0; i < total; ++i) base[i] = uint8_t(0xA0 + i % 7);
    hipStream_t st = nullptr;
    for (int k = 0; k < 5; ++k) switch ((k + rot) % 4) {
            case 0: check_section(a, s1[k], base, total, st); break;
            case 1: check_section(a, s4[k], base, total, st); break;
            case 2: check_section(a, s8[k], base, total, st); break;
            default: check_section(a, s24[k], base, total, st); break;
        }
}

// ---- the row cutter
struct PlainRow {
    uint64_t src, dst;
    uint32_t len;
};
KVStore table_of(uint32_t key_base, const std::vector<uint64_t>& row_lens) {
    KVStore t;
    t.key_base = key_base;
    t.num_keys = uint32_t(row_lens.size());
    t.host_off.assign(1, 0);
    for (uint64_t l : row_lens) t.host_off.push_back(t.host_off.back() + l);
    return t;
}
long check_row_cutter() {
    // rows of 0, 1, 65535, 65536, 65537 and 131073 entries behind key base 10; a second table with its own rows
    const KVStore t1 = table_of(10, {0, 1, 65535, 65536, 65537, 131073, 7}), t2 = table_of(0, {3, 0, 70000});
    struct Job {
        const KVStore* table;
        std::vector<uint32_t> keys;
    };
    const std::vector<Job> jobs = {
        {&t1, {9, 10, 11, 12, 13, 14, 15, 17, 16}},  // 9: below key_base; 17: key_base + num_keys; 16: the last key
        {&t1, {15, 15, 11, 1000000}},                  // the second job on the same table: a row twice
        {&t2, {2, 0, 1, 3}},                           // another table
    };
    GatherStage g;
    std::vector<PlainRow> rows;
    std::vector<uint32_t> sb, se;
    std::vector<std::pair<size_t, size_t>> table_rows;
    uint64_t cursor = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {
        const KVStore& t = *jobs[j].table;
        const bool new_table = j == 0 || jobs[j].table != jobs[j - 1].table;
        g.add_job(t, new_table, jobs[j].keys, "too many entries");
        // the plain loop
        if (new_table) table_rows.push_back({rows.size(), rows.size()});
        sb.push_back(uint32_t(cursor));
        for (uint32_t key : jobs[j].keys) {
            if (key < t.key_base || key >= uint64_t(t.key_base) + t.num_keys) continue;
            const uint64_t begin = t.host_off[key - t.key_base], end = t.host_off[key - t.key_base + 1];
            for (uint64_t at = begin; at < end; at += 65536) {
                const uint32_t len = uint32_t(end - at < 65536 ? end - at : 65536);
                rows.push_back({at, cursor, len});
                cursor += len;
            }
        }
        se.push_back(uint32_t(cursor));
        table_rows.back().second = rows.size();
        CHECK(g.cursor == cursor);
    }
    CHECK(g.rows.size() == rows.size() && g.seg_begin == sb && g.seg_end == se && g.table_rows == table_rows && g.table_vals.size() == 2);
    StageArena m;  // the stage's own sections: [rows][seg_begin][seg_end] behind the caller's jobs table
    const auto s_jobs = m.add<uint64_t>(jobs.size());
    g.layout(m);
    CHECK(s_jobs.off == 0 && g.s_rows.off == 256 && g.s_rows.n == rows.size() && g.s_begin.n == jobs.size() && g.s_end.n == jobs.size() &&
          g.s_begin.off == 256 + (rows.size() * sizeof(LocRow) + 255) / 256 * 256 && g.s_end.off == g.s_begin.off + 256);
    for (size_t r = 0; r < rows.size(); ++r)
        CHECK(g.rows[r].src == rows[r].src && g.rows[r].dst == rows[r].dst && g.rows[r].len == rows[r].len && g.rows[r].pad == 0 && rows[r].len >= 1 && rows[r].len <= 65536);
    // what the shapes are there for: 65536 stays one piece, 65537 is 65536 + 1, 131073 is 65536 + 65536 + 1; the keys outside gather nothing
    CHECK(rows.size() == 1 + 1 + 1 + 2 + 3 + 1 + (3 + 3 + 1) + (2 + 1) && rows[2].len == 65536 && rows[4].len == 1 && rows[7].len == 1);
    CHECK(table_rows.size() == 2 && table_rows[0] == std::make_pair(size_t(0), size_t(16)) && table_rows[1] == std::make_pair(size_t(16), size_t(19)));
    CHECK(se[0] == 1 + 65535 + 65536 + 65537 + 131073 + 7 && sb[1] == se[0] && se[2] - sb[2] == 70003);
    // a job without any row: an empty slice, no piece
    GatherStage none;
    none.add_job(t1, true, {9, 10, 17}, "too many entries");
    CHECK(none.rows.empty() && none.cursor == 0 && none.seg_begin == std::vector<uint32_t>{0} && none.seg_end == std::vector<uint32_t>{0} &&
          none.table_rows.size() == 1 && none.table_rows[0].first == 0 && none.table_rows[0].second == 0);
    return long(rows.size());
}
}  // namespace

int main() {
    const int orders[4][5] = {{0, 1, 2, 3, 4}, {4, 3, 2, 1, 0}, {2, 0, 4, 1, 3}, {3, 4, 0, 2, 1}};
    for (const auto& order : orders)
        for (int rot = 0; rot < 4; ++rot) check_arena(order, rot, rot == 1 ? 16 : rot == 2 ? 256 : 0);
    // an arena of empty sections only: commits, copies nothing
    {
        StageArena a;
        const auto s = a.add<uint64_t>(0);
        DevBuf buf;
        a.commit(buf, 16);
        const long calls = vq_stub_async_calls();
        a.upload(s, static_cast<const uint64_t*>(nullptr), nullptr);
        a.zero(s, nullptr);
        a.download(s, static_cast<uint64_t*>(nullptr), nullptr);
        CHECK(vq_stub_async_calls() == calls && a.whole().n == 0 && buf.bytes >= 16);
    }
    const long pieces = check_row_cutter();
    for (uint64_t len : {0ull, 1ull, 3ull, 4ull, 5ull, 0xFFFFFFF0ull}) {
        const uint64_t want = (len + 8 + 3) / 4 * 4;  // in 64 bits
        CHECK(padded_list_len(len) == want && want % 4 == 0 && want >= len + 8 && want < len + 12);
    }
    CHECK(padded_list_len(0xFFFFFFF0ull) == 0xFFFFFFF8ull && padded_list_len(0) == 8 && padded_list_len(5) == 16);
    CHECK(value_of_order_key(order_f32(0x40490FDBu)) == 3.14159274f && value_of_order_key(order_f32(0xBF800000u)) == -1.0f);
    std::printf("STAGING_CHECK_OK {\"arenas\": %ld, \"sections\": %ld, \"row_pieces\": %ld}\n", g_arenas, g_sections, pieces);
    return 0;
}
