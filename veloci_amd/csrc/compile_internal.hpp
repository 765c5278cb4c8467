// What compile.cpp, term_lookup.cpp and text_requests.cpp share and nobody else needs: the decline, the phase timer, two path helpers.
#pragma once
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"

namespace vq {
// thread-time per compilation phase (defined in compile.cpp, printed per batch by exec.cpp): 0 lookup_terms (term_lookup.cpp), 1 resolve_boost_1n,
// 2 emit_boost_1n rest, 3 leaf lists, 4 the longest single compile_query, 5 total; inside 1: 6 value-id gather, 7 sort, 8 (anchor, value) pairs;
// 9 order check + layers of a resolved list
extern std::atomic<uint64_t> g_compile_ns[16];

inline bool ends_with(const std::string& s, const char* suf) {
    size_t n = std::strlen(suf);
    return s.size() >= n && std::memcmp(s.data() + s.size() - n, suf, n) == 0;
}

[[noreturn]] inline void unsupported(const std::string& what) {
    throw VelociError(vqreq::ERR_UNSUPPORTED, "unsupported on the MI355X query path: " + what);
}

// reference src/util.rs:147-162
inline std::vector<std::string> get_steps_to_anchor(const std::string& path) {
    std::vector<std::string> paths;
    std::string current;
    size_t start = 0;
    while (true) {
        size_t dot = path.find('.', start);
        std::string part = path.substr(start, dot == std::string::npos ? std::string::npos : dot - start);
        if (!current.empty()) current += ".";
        current += part;
        if (ends_with(part, "[]")) paths.push_back(current);
        if (dot == std::string::npos) break;
        start = dot + 1;
    }
    paths.push_back(path + TEXTINDEX);
    return paths;
}

// VQ_TIMING: where request compilation spends its time (summed over threads, printed per batch by exec.cpp)
struct PhaseTimer {
    static bool on() {
        static const bool v = std::getenv("VQ_TIMING") != nullptr;
        return v;
    }
    int slot;
    std::chrono::steady_clock::time_point t0;
    explicit PhaseTimer(int s) : slot(s) {
        if (on()) t0 = std::chrono::steady_clock::now();
    }
    ~PhaseTimer() {
        if (!on()) return;
        const uint64_t ns = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
        g_compile_ns[slot] += ns;
        if (slot == 5) {  // the longest single request: what bounds a parallel pass from below
            uint64_t cur = g_compile_ns[4].load();
            while (ns > cur && !g_compile_ns[4].compare_exchange_weak(cur, ns)) {
            }
        }
    }
};
}  // namespace vq
