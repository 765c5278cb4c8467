// TEST PROGRAM (tests/test_regex_dfa_cpu.py builds it with g++ -fsanitize=address,undefined next to veloci_amd/csrc/regex_dfa.cpp and runs it):
// the pattern -> DFA compiler of the device regex route against its yardstick, std::wregex as regex_candidates (term_lookup.cpp) uses it.
//   1. seeded random patterns from the supported grammar (every operator, groups nested to depth 3, repeats bounded so that the state cap is out
//      of reach) x random terms of 0..20 code points over three alphabets (ASCII; Latin-1 + Greek; one with code points above U+FFFF), for
//      ignore_case x starts_with: walking the DFA must agree with regex_match of `[\s\S]*?(?:pattern)` / regex_search of the pattern.
//      Zero disagreements, zero generated patterns declined.
//   2. a fixed list of patterns outside the grammar: each is declined with a reason.
// usage: regex_dfa_check [patterns per alphabet] [terms per pattern] [seed]; prints one summary line, exit status 0 when every condition holds.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <regex>
#include <string>
#include <vector>

#include "../../veloci_amd/csrc/regex_dfa.hpp"
#include "../../veloci_amd/csrc/text.hpp"

namespace {

using Cps = std::vector<uint32_t>;
std::mt19937_64 rng;
uint32_t pick(uint32_t n) { return uint32_t(rng() % n); }

struct Alphabet {
    const char* name;
    Cps all;      // sorted, distinct: what the dictionary holds
    Cps letters;  // what literals and terms are mostly drawn from
};

Alphabet make_ascii() {
    Alphabet a{"ascii", {}, {}};
    for (uint32_t c = 32; c < 127; ++c) a.all.push_back(c);
    a.all.insert(a.all.begin(), {9u, 10u, 13u});
    for (uint32_t c : Cps{'a', 'b', 'c', 'A', 'B', 'x', 'Z', '0', '7', '_', ' ', '.', '*', '-', '\n', '(', ']', '\\', '|', '^'}) a.letters.push_back(c);
    return a;
}
Alphabet make_latin_greek() {
    Alphabet a{"latin1+greek", {}, {}};
    for (uint32_t c : Cps{10u, 32u, '0', '5', 'a', 'b', 'e', 'E', 'k', 'K', 's', 'S', '_'}) a.all.push_back(c);
    for (uint32_t c = 0xA0; c <= 0xFF; ++c) a.all.push_back(c);
    for (uint32_t c = 0x386; c <= 0x3CE; ++c)
        if (c != 0x38B && c != 0x38D && c != 0x3A2) a.all.push_back(c);
    a.all.push_back(0x2028);  // `.` rejects it
    a.all.push_back(0x212A);  // KELVIN SIGN
    // (U+00E9 / U+00C9, U+00DF, U+00B5 / U+03BC, sigma and final sigma, U+00FF: the cases a restated icase rule gets wrong)
    a.letters = {'a', 'e', 'E', 'k', 's', 0xE9, 0xC9, 0xDF, 0xB5, 0x3BC, 0x3C3, 0x3C2, 0x3A3, 0x3B1, 0x391, 0xFF, 0xA0, 0x2028, 0x212A, '5', '_'};
    return a;
}
Alphabet make_astral() {
    Alphabet a{"astral", {}, {}};
    for (uint32_t c : Cps{10u, 32u, '1', 'a', 'A', 'b', 'z', 0xE9, 0x3B1, 0x4E2D, 0xFFFD}) a.all.push_back(c);
    for (uint32_t c = 0x10400; c <= 0x1044F; ++c) a.all.push_back(c);  // Deseret: cased, above U+FFFF
    for (uint32_t c = 0x1F600; c <= 0x1F60F; ++c) a.all.push_back(c);
    a.all.push_back(0x10FFFF);
    a.letters = {'a', 'A', 'b', '1', 0x10400, 0x10428, 0x10401, 0x1F600, 0x1F60A, 0x4E2D, 0x10FFFF, 0xE9, ' '};
    return a;
}

bool special(uint32_t c) { return c < 128 && std::string("\\^$.|?*+()[]{}").find(char(c)) != std::string::npos; }
void literal(Cps& out, uint32_t c) {
    if (c == '\n' && pick(2)) {
        out.push_back('\\');
        out.push_back('n');
        return;
    }
    if (special(c) || (c < 128 && c > 32 && !isalnum(int(c)) && c != '_' && pick(3) == 0)) out.push_back('\\');  // escaped literals, needed or not
    out.push_back(c);
}

// `width`: an upper bound of the characters the expression consumes along one path, with `*` / `+` / `{m,}` counted by their mandatory part + 1:
// with the unanchored prefix the DFA has at most about 2^width states
struct Gen {
    const Alphabet& A;
    Cps hot;
    uint32_t hot_cp() { return hot[pick(uint32_t(hot.size()))]; }
    uint32_t bracket_cp() {  // bracket members: no character that means something inside brackets
        for (;;) {
            const uint32_t c = pick(4) ? hot_cp() : A.all[pick(uint32_t(A.all.size()))];
            if (c >= 128 || isalnum(int(c))) return c;
        }
    }
    uint32_t atom(Cps& out) {
        switch (pick(10)) {
            case 0: out.push_back('.'); break;
            case 1: {
                out.push_back('\\');
                out.push_back(uint32_t("dDwWsS"[pick(6)]));
                break;
            }
            case 2: case 3: {
                out.push_back('[');
                if (pick(3) == 0) out.push_back('^');
                const uint32_t n = 1 + pick(3);
                for (uint32_t k = 0; k < n; ++k) {
                    const uint32_t kind = pick(5);
                    if (kind == 0) {
                        out.push_back('\\');
                        out.push_back(uint32_t("dws"[pick(3)]));
                    } else if (kind == 1) {
                        uint32_t lo = bracket_cp(), hi = bracket_cp();
                        if (lo > hi) std::swap(lo, hi);
                        out.push_back(lo);
                        out.push_back('-');
                        out.push_back(hi);
                    } else out.push_back(bracket_cp());
                }
                out.push_back(']');
                break;
            }
            default: literal(out, pick(8) ? hot_cp() : A.all[pick(uint32_t(A.all.size()))]);
        }
        return 1;
    }
    // (std::wregex's matcher backtracks: an unbounded repeat over a group that itself holds a repeat or an alternation takes exponential time on
    //  terms that do not match, so such groups get a bounded repeat here; `plain` = neither inside)
    struct Info {
        uint32_t w;
        bool plain;
    };
    Info quantified(Cps& out, int depth, uint32_t budget) {
        Cps inner;
        Info in{1, true};
        const bool group = depth < 3 && pick(3) == 0;
        if (group) {
            inner.push_back('(');
            if (pick(2)) {
                inner.push_back('?');
                inner.push_back(':');
            }
            in = alternation(inner, depth + 1, budget);
            inner.push_back(')');
        } else atom(inner);
        uint32_t lo = 1, hi = 1;
        std::string q;
        switch (pick(9)) {
            case 0: q = "*"; lo = 0; hi = 0xFFFF; break;
            case 1: q = "+"; lo = 1; hi = 0xFFFF; break;
            case 2: q = "?"; lo = 0; hi = 1; break;
            case 3: lo = hi = pick(4); q = "{" + std::to_string(lo) + "}"; break;
            case 4: lo = pick(3); hi = 0xFFFF; q = "{" + std::to_string(lo) + ",}"; break;
            case 5: lo = pick(3); hi = lo + pick(3); q = "{" + std::to_string(lo) + "," + std::to_string(hi) + "}"; break;
            default: break;
        }
        if (hi == 0xFFFF && !in.plain) {
            hi = lo + 2;
            q = "{" + std::to_string(lo) + "," + std::to_string(hi) + "}";
        }
        const uint32_t copies = hi == 0xFFFF ? lo + 1 : hi;
        if (in.w * copies > budget) q.clear();
        else if (!q.empty() && pick(3) == 0) q += '?';  // lazy
        out.insert(out.end(), inner.begin(), inner.end());
        for (char c : q) out.push_back(uint32_t(c));
        return {q.empty() ? in.w : in.w * copies, in.plain && q.empty()};
    }
    Info sequence(Cps& out, int depth, uint32_t budget) {
        if (pick(12) == 0) return {0, true};  // an empty branch
        Info s{0, true};
        const uint32_t n = 1 + pick(4);
        for (uint32_t k = 0; k < n && s.w < budget; ++k) {
            const Info t = quantified(out, depth, budget - s.w);
            s.w += t.w;
            s.plain = s.plain && t.plain;
        }
        return s;
    }
    Info alternation(Cps& out, int depth, uint32_t budget) {
        Info a = sequence(out, depth, budget);
        const uint32_t extra = pick(4) == 0 ? 1 + pick(2) : 0;
        for (uint32_t k = 0; k < extra; ++k) {
            out.push_back('|');
            a.w += sequence(out, depth, budget - std::min(a.w, budget)).w;  // (the branches' positions add up in the subset construction)
            a.plain = false;
        }
        return a;
    }
};

std::wstring widen(const Cps& c) {
    std::wstring w;
    for (uint32_t cp : c) w.push_back(wchar_t(cp));
    return w;
}
std::string utf8(const Cps& c) {
    std::string s;
    for (uint32_t cp : c) vqtext::append_utf8(s, cp);
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    const uint32_t n_patterns = argc > 1 ? uint32_t(std::atoi(argv[1])) : 700u, n_terms = argc > 2 ? uint32_t(std::atoi(argv[2])) : 200u;
    rng.seed(argc > 3 ? uint64_t(std::atoll(argv[3])) : 20240611ull);
    Alphabet alphabets[3] = {make_ascii(), make_latin_greek(), make_astral()};
    for (Alphabet& A : alphabets) {
        std::sort(A.all.begin(), A.all.end());
        A.all.erase(std::unique(A.all.begin(), A.all.end()), A.all.end());
        for (uint32_t c : A.letters)
            if (!std::binary_search(A.all.begin(), A.all.end(), c)) return std::printf("letter U+%04X outside its alphabet\n", c), 2;
    }
    uint64_t patterns = 0, compared = 0, disagreements = 0, declined = 0, invalid = 0, accepted = 0, max_states = 0, operators[8] = {};
    for (const Alphabet& A : alphabets) {
        vqregex::AtomCache cache;
        for (uint32_t pi = 0; pi < n_patterns; ++pi) {
            Gen g{A, {}};
            for (int k = 0; k < 5; ++k) g.hot.push_back(A.letters[pick(uint32_t(A.letters.size()))]);
            Cps pat;
            // the first few: repeats over alternations and stacked quantifiers, which the generator keeps bounded
            static const char* const kFixed[] = {"(foo|ba[rz])+x?", "(ab|cd)*e", "(a|b)*abb", "a*+b", "a{2}{2}", "a*??b", "(a|)+b", "ab.*", "[a-c]{2,3}d.*e", ".*[a-g]", "()", "a||b"};
            if (pi < sizeof kFixed / sizeof kFixed[0]) pat = vqtext::decode_utf8(std::string(kFixed[pi]));
            else g.alternation(pat, 0, 9);
            for (uint32_t c : pat) {
                const char* ops = "*+?{|([";
                for (int o = 0; ops[o]; ++o) operators[o] += c == uint32_t(ops[o]);
            }
            std::vector<Cps> terms(n_terms);
            for (Cps& t : terms) {
                const uint32_t len = pick(21);
                for (uint32_t k = 0; k < len; ++k) t.push_back(pick(5) ? g.hot_cp() : A.all[pick(uint32_t(A.all.size()))]);
            }
            ++patterns;
            const auto t_begin = std::chrono::steady_clock::now();
            double compile_s = 0;
            for (int icase = 0; icase < 2; ++icase) {
                std::wregex whole, anywhere;
                try {
                    const auto flags = std::regex::ECMAScript | (icase ? std::regex::icase : std::regex::ECMAScript);
                    whole = std::wregex(L"[\\s\\S]*?(?:" + widen(pat) + L")", flags);
                    anywhere = std::wregex(widen(pat), flags);
                } catch (const std::regex_error& e) {
                    ++invalid;
                    std::printf("INVALID %s: %s\n", utf8(pat).c_str(), e.what());
                    continue;
                }
                for (int sw = 0; sw < 2; ++sw) {
                    const auto c_begin = std::chrono::steady_clock::now();
                    const vqregex::Compiled c = vqregex::compile(pat, icase != 0, sw != 0, A.all, cache);
                    compile_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - c_begin).count();
                    if (!c.device) {
                        ++declined;
                        std::printf("DECLINED %s: %s\n", utf8(pat).c_str(), c.reason.c_str());
                        continue;
                    }
                    max_states = std::max<uint64_t>(max_states, c.dfa.n_states);
                    for (const Cps& t : terms) {
                        const std::wstring w = widen(t);
                        const bool want = sw ? std::regex_search(w, anywhere) : std::regex_match(w, whole);
                        const bool got = vqregex::accepts(c.dfa, A.all, t.data(), t.size());
                        ++compared;
                        accepted += want;
                        if (want != got && ++disagreements <= 20)
                            std::printf("DISAGREE [%s] pattern %s term %s icase %d starts_with %d: std::wregex %d, DFA %d\n", A.name, utf8(pat).c_str(), utf8(t).c_str(), icase, sw,
                                        int(want), int(got));
                    }
                }
            }
            const double took = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
            if (took > 2.0) std::printf("SLOW %.1f s (compiling: %.1f s) [%s] pattern %s\n", took, compile_s, A.name, utf8(pat).c_str()), std::fflush(stdout);
        }
    }
    // outside the grammar: declined with a reason, whatever std::wregex makes of them
    const char* outside[] = {"(a)\\1", "a(?=b)", "a(?!b)", "^ab", "ab$", "a^b", "\\bab", "a\\Bb", "[[:alpha:]]+", "[[.a.]]", "[[=a=]]", "a[]b", "a[^]b", ".*a.{13}",
                             "\\x41", "\\u0041", "\\cA", "\\p", "a{40000}", "(?<n>a)"};
    uint64_t not_declined = 0;
    vqregex::AtomCache cache;
    for (const char* p : outside) {
        const vqregex::Compiled c = vqregex::compile(vqtext::decode_utf8(std::string(p)), true, false, alphabets[0].all, cache);
        if (c.device || c.reason.empty()) {
            ++not_declined;
            std::printf("NOT DECLINED %s\n", p);
        }
    }
    bool every_operator = true;
    for (int o = 0; o < 7; ++o) every_operator = every_operator && operators[o] > 0;
    std::printf("REGEX_DFA_CHECK {\"patterns\":%llu,\"terms_per_pattern\":%u,\"compared\":%llu,\"accepted\":%llu,\"disagreements\":%llu,\"declined\":%llu,\"invalid\":%llu,"
                "\"max_states\":%llu,\"outside\":%zu,\"outside_not_declined\":%llu,\"every_operator\":%s}\n",
                (unsigned long long)patterns, n_terms, (unsigned long long)compared, (unsigned long long)accepted, (unsigned long long)disagreements,
                (unsigned long long)declined, (unsigned long long)invalid, (unsigned long long)max_states, sizeof outside / sizeof outside[0],
                (unsigned long long)not_declined, every_operator ? "true" : "false");
    return disagreements || declined || invalid || not_declined || !every_operator ? 1 : 0;
}
