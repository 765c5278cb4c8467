// Pattern -> DFA over the code points of one dictionary (regex_dfa.hpp).  Parser of the supported structure, Thompson construction, subset
// construction over the alphabet's equivalence classes.
#include "regex_dfa.hpp"

#include <algorithm>
#include <regex>
#include <unordered_map>

namespace vqregex {
namespace {

struct Decline {  // thrown inside compile(): the pattern stays on the host route
    std::string why;
};

struct Node {
    enum Kind { Empty, Atom, Cat, Alt, Rep } kind = Empty;
    uint32_t atom = 0;         // Atom: index into Parser::atoms
    std::vector<int> kids;     // Cat / Alt; Rep: one
    uint32_t lo = 0, hi = 0;   // Rep: hi == kInf: no upper bound
};
constexpr uint32_t kInf = 0xFFFFFFFFu;
constexpr int kMaxDepth = 200;  // nested groups
constexpr int kMaxStacked = 8;  // quantifiers behind one atom (`a*?+{2}`): bounds the recursion over the tree

struct Parser {
    const std::vector<uint32_t>& p;
    size_t i = 0;
    int depth = 0;
    std::vector<Node> nodes;
    std::vector<std::wstring> atoms;  // distinct atom texts
    std::map<std::wstring, uint32_t> atom_ids;

    explicit Parser(const std::vector<uint32_t>& pattern) : p(pattern) {}
    bool at_end() const { return i >= p.size(); }
    int add(Node n) {
        nodes.push_back(std::move(n));
        return int(nodes.size()) - 1;
    }
    int atom_node(const std::wstring& text) {
        auto it = atom_ids.find(text);
        if (it == atom_ids.end()) {
            it = atom_ids.emplace(text, uint32_t(atoms.size())).first;
            atoms.push_back(text);
        }
        Node n;
        n.kind = Node::Atom;
        n.atom = it->second;
        return add(std::move(n));
    }
    int parse() {
        const int root = alternation();
        if (!at_end()) throw Decline{"unbalanced `)`"};
        return root;
    }
    int alternation() {
        Node alt;
        alt.kind = Node::Alt;
        alt.kids.push_back(sequence());
        while (!at_end() && p[i] == '|') {
            ++i;
            alt.kids.push_back(sequence());
        }
        if (alt.kids.size() == 1) return alt.kids[0];
        return add(std::move(alt));
    }
    int sequence() {  // may be empty: `a|`, `()`
        Node cat;
        cat.kind = Node::Cat;
        while (!at_end() && p[i] != '|' && p[i] != ')') cat.kids.push_back(term());
        if (cat.kids.empty()) return add(Node{});
        if (cat.kids.size() == 1) return cat.kids[0];
        return add(std::move(cat));
    }
    int term() {
        int n = atom();
        for (int stacked = 0; !at_end(); ++stacked) {  // libstdc++ takes any number of quantifiers behind an atom, each over all that precedes it
            uint32_t lo, hi;
            const uint32_t c = p[i];
            if (c == '*') lo = 0, hi = kInf, ++i;
            else if (c == '+') lo = 1, hi = kInf, ++i;
            else if (c == '?') lo = 0, hi = 1, ++i;
            else if (c == '{') {
                ++i;
                lo = number();
                hi = lo;
                if (!at_end() && p[i] == ',') {
                    ++i;
                    hi = (!at_end() && p[i] >= '0' && p[i] <= '9') ? number() : kInf;
                }
                if (at_end() || p[i] != '}') throw Decline{"malformed `{m,n}`"};
                ++i;
                if (hi < lo) throw Decline{"malformed `{m,n}`"};
            } else break;
            if (stacked >= kMaxStacked) throw Decline{"more than " + std::to_string(kMaxStacked) + " quantifiers behind one atom"};
            if (!at_end() && p[i] == '?') ++i;  // lazy: which match is found changes, not whether there is one
            Node r;
            r.kind = Node::Rep;
            r.kids.push_back(n);
            r.lo = lo;
            r.hi = hi;
            n = add(std::move(r));
        }
        return n;
    }
    uint32_t number() {
        if (at_end() || p[i] < '0' || p[i] > '9') throw Decline{"malformed `{m,n}`"};
        uint64_t v = 0;
        while (!at_end() && p[i] >= '0' && p[i] <= '9') {
            v = v * 10 + (p[i++] - '0');
            if (v > kMaxNfaStates) throw Decline{"a repeat count above " + std::to_string(kMaxNfaStates)};
        }
        return uint32_t(v);
    }
    int atom() {
        const uint32_t c = p[i];
        switch (c) {
            case '(': {
                ++i;
                if (!at_end() && p[i] == '?') {
                    if (i + 1 < p.size() && p[i + 1] == ':') i += 2;
                    else if (i + 1 < p.size() && (p[i + 1] == '=' || p[i + 1] == '!')) throw Decline{"look-ahead `(?=` / `(?!`"};
                    else throw Decline{"a group the compiler does not know: `(?`"};
                }
                if (++depth > kMaxDepth) throw Decline{"groups nested deeper than " + std::to_string(kMaxDepth)};
                const int n = alternation();
                --depth;
                if (at_end() || p[i] != ')') throw Decline{"unbalanced `(`"};
                ++i;
                return n;
            }
            case '[': return bracket();
            case '\\': return escape();
            case '.': ++i; return atom_node(L".");
            case '^': throw Decline{"anchor `^`"};
            case '$': throw Decline{"anchor `$`"};
            case '*': case '+': case '?': case '{': throw Decline{"a quantifier with nothing to repeat"};
            case ']': case '}': throw Decline{"a stray `]` or `}`"};
            default: ++i; return atom_node(std::wstring(1, wchar_t(c)));
        }
    }
    int escape() {
        if (i + 1 >= p.size()) throw Decline{"a trailing backslash"};
        const uint32_t e = p[i + 1];
        if (e >= '1' && e <= '9') throw Decline{"back-reference"};
        if (e == 'b' || e == 'B') throw Decline{"word boundary `\\b` / `\\B`"};
        const bool cls = e == 'd' || e == 'D' || e == 'w' || e == 'W' || e == 's' || e == 'S';
        const bool ctl = e == 'f' || e == 'n' || e == 'r' || e == 't' || e == 'v' || e == '0';
        const bool punct = e < 128u && e > 32u && !((e >= '0' && e <= '9') || (e >= 'a' && e <= 'z') || (e >= 'A' && e <= 'Z') || e == '_');
        if (!cls && !ctl && !punct) throw Decline{"an escape the compiler does not know"};
        std::wstring text{L'\\', wchar_t(e)};
        i += 2;
        return atom_node(text);
    }
    int bracket() {  // verbatim up to the closing `]`: what it matches is std::wregex's answer
        const size_t b = i++;
        if (!at_end() && p[i] == '^') ++i;
        if (!at_end() && p[i] == ']') throw Decline{"the bracket forms `[]` / `[^]`"};
        for (;;) {
            if (at_end()) throw Decline{"an unclosed bracket expression"};
            const uint32_t c = p[i];
            if (c == '\\') {
                if (i + 1 >= p.size()) throw Decline{"an unclosed bracket expression"};
                i += 2;
            } else if (c == '[' && i + 1 < p.size() && (p[i + 1] == ':' || p[i + 1] == '.' || p[i + 1] == '=')) {
                throw Decline{"a bracket expression with `[:`, `[.` or `[=`"};
            } else if (c == ']') {
                ++i;
                break;
            } else ++i;
        }
        std::wstring text;
        for (size_t k = b; k < i; ++k) text.push_back(wchar_t(p[k]));
        return atom_node(text);
    }
};

// Thompson NFA: state s has up to one labelled edge (atom `label[s]`, or kAny: every character) to `to[s]`, and epsilon edges
constexpr uint32_t kNoLabel = 0xFFFFFFFFu, kAny = 0xFFFFFFFEu;
struct Nfa {
    std::vector<uint32_t> label, to;
    std::vector<std::vector<uint32_t>> eps;
    uint32_t state() {
        if (label.size() >= kMaxNfaStates) throw Decline{"a pattern that expands to more than " + std::to_string(kMaxNfaStates) + " NFA states"};
        label.push_back(kNoLabel);
        to.push_back(0);
        eps.emplace_back();
        return uint32_t(label.size()) - 1;
    }
};
struct Frag {
    uint32_t in, out;
};
struct Builder {
    const std::vector<Node>& nodes;
    Nfa& nfa;
    Frag emit(int id) {
        const Node& n = nodes[size_t(id)];
        switch (n.kind) {
            case Node::Empty: {
                const uint32_t s = nfa.state();
                return {s, s};
            }
            case Node::Atom: {
                const uint32_t a = nfa.state(), b = nfa.state();
                nfa.label[a] = n.atom;
                nfa.to[a] = b;
                return {a, b};
            }
            case Node::Cat: {
                Frag f = emit(n.kids[0]);
                for (size_t k = 1; k < n.kids.size(); ++k) {
                    const Frag g = emit(n.kids[k]);
                    nfa.eps[f.out].push_back(g.in);
                    f.out = g.out;
                }
                return f;
            }
            case Node::Alt: {
                const uint32_t a = nfa.state(), b = nfa.state();
                for (int k : n.kids) {
                    const Frag g = emit(k);
                    nfa.eps[a].push_back(g.in);
                    nfa.eps[g.out].push_back(b);
                }
                return {a, b};
            }
            case Node::Rep: {
                const uint32_t a = nfa.state();
                uint32_t cur = a;
                for (uint32_t k = 0; k < n.lo; ++k) {  // the mandatory copies
                    const Frag g = emit(n.kids[0]);
                    nfa.eps[cur].push_back(g.in);
                    cur = g.out;
                }
                if (n.hi == kInf) {  // ... then any number more
                    const uint32_t loop = nfa.state();
                    nfa.eps[cur].push_back(loop);
                    const Frag g = emit(n.kids[0]);
                    nfa.eps[loop].push_back(g.in);
                    nfa.eps[g.out].push_back(loop);
                    return {a, loop};
                }
                const uint32_t end = nfa.state();
                for (uint32_t k = n.lo; k < n.hi; ++k) {  // ... then up to hi - lo optional ones
                    nfa.eps[cur].push_back(end);
                    const Frag g = emit(n.kids[0]);
                    nfa.eps[cur].push_back(g.in);
                    cur = g.out;
                }
                nfa.eps[cur].push_back(end);
                return {a, end};
            }
        }
        return {0, 0};
    }
};

// which code points of the alphabet `atom` matches: std::wregex's own answer, one one-character regex_match per code point
std::shared_ptr<const std::vector<uint8_t>> atom_members(const std::wstring& atom, bool icase, const std::vector<uint32_t>& alphabet, AtomCache& cache) {
    const auto key = std::make_pair(atom, icase);
    {
        std::lock_guard<std::mutex> g(cache.mu);
        auto it = cache.members.find(key);
        if (it != cache.members.end()) return it->second;
    }
    std::wregex re;
    try {
        re = std::wregex(atom, std::regex::ECMAScript | (icase ? std::regex::icase : std::regex::ECMAScript));
    } catch (const std::regex_error& e) {
        throw Decline{std::string("an atom std::wregex does not take on its own (") + e.what() + ")"};
    }
    auto m = std::make_shared<std::vector<uint8_t>>(alphabet.size());
    std::wstring one(1, L' ');
    for (size_t k = 0; k < alphabet.size(); ++k) {
        one[0] = wchar_t(alphabet[k]);
        (*m)[k] = std::regex_match(one, re) ? 1 : 0;
    }
    std::lock_guard<std::mutex> g(cache.mu);
    return cache.members.emplace(key, std::move(m)).first->second;
}

struct VecHash {
    size_t operator()(const std::vector<uint32_t>& v) const {
        uint64_t h = 0xcbf29ce484222325ull;
        for (uint32_t x : v) h = (h ^ x) * 0x100000001b3ull;
        return size_t(h);
    }
};

}  // namespace

Compiled compile(const std::vector<uint32_t>& pattern, bool icase, bool starts_with, const std::vector<uint32_t>& alphabet, AtomCache& cache) {
    Compiled out;
    try {
        if (alphabet.size() > kMaxAlphabet) throw Decline{"a dictionary alphabet of more than " + std::to_string(kMaxAlphabet) + " code points"};
        Parser parser(pattern);
        const int root = parser.parse();

        // equivalence classes of the alphabet: code points no atom of this pattern tells apart
        std::vector<std::shared_ptr<const std::vector<uint8_t>>> members;
        for (const std::wstring& a : parser.atoms) members.push_back(atom_members(a, icase, alphabet, cache));
        Dfa& dfa = out.dfa;
        dfa.cls.resize(alphabet.size());
        std::vector<uint32_t> class_rep;  // an index into the alphabet per class
        {
            std::map<std::vector<uint8_t>, uint32_t> by_signature;
            std::vector<uint8_t> sig(members.size());
            for (size_t k = 0; k < alphabet.size(); ++k) {
                for (size_t a = 0; a < members.size(); ++a) sig[a] = (*members[a])[k];
                auto it = by_signature.find(sig);
                if (it == by_signature.end()) {
                    it = by_signature.emplace(sig, uint32_t(class_rep.size())).first;
                    class_rep.push_back(uint32_t(k));
                }
                dfa.cls[k] = uint16_t(it->second);
            }
        }
        const uint32_t C = std::max<uint32_t>(uint32_t(class_rep.size()), 1u);  // (an empty alphabet: one class nobody is in)
        uint32_t non_ascii = 0;
        for (uint32_t cp : alphabet) non_ascii += cp >= 128u;

        // "any characters, then the pattern"
        Nfa nfa;
        const uint32_t any = nfa.state();
        nfa.label[any] = kAny;
        nfa.to[any] = any;
        Builder builder{parser.nodes, nfa};
        const Frag f = builder.emit(root);
        nfa.eps[any].push_back(f.in);
        const uint32_t accept = f.out;

        // subset construction over the classes
        std::vector<uint32_t> stamp(nfa.label.size(), 0u), stack;
        uint32_t round = 0;
        auto close = [&](std::vector<uint32_t>& set) {  // epsilon closure, sorted; with starts_with an accepting set is the one absorbing state
            ++round;
            stack.assign(set.begin(), set.end());
            set.clear();
            for (uint32_t s : stack) stamp[s] = round;
            while (!stack.empty()) {
                const uint32_t s = stack.back();
                stack.pop_back();
                set.push_back(s);
                for (uint32_t t : nfa.eps[s])
                    if (stamp[t] != round) {
                        stamp[t] = round;
                        stack.push_back(t);
                    }
            }
            if (starts_with && stamp[accept] == round) set.assign(1, accept);
            else std::sort(set.begin(), set.end());
        };
        std::unordered_map<std::vector<uint32_t>, uint32_t, VecHash> ids;
        std::vector<std::vector<uint32_t>> sets;
        std::vector<uint16_t> next;
        auto id_of = [&](std::vector<uint32_t>& set) {
            auto it = ids.find(set);
            if (it != ids.end()) return it->second;
            if (sets.size() >= kMaxStates) throw Decline{"a DFA of more than " + std::to_string(kMaxStates) + " states"};
            if (lds_table_bytes(sets.size() + 1, C, non_ascii) > kLdsTableBytes)
                throw Decline{"tables of " + std::to_string(sets.size() + 1) + "+ states x " + std::to_string(C) + " classes and " + std::to_string(non_ascii) +
                              " non-ASCII code points: more than the kernel's LDS table budget of " + std::to_string(kLdsTableBytes) + " bytes"};
            const uint32_t id = uint32_t(sets.size());
            ids.emplace(set, id);
            sets.push_back(set);
            return id;
        };
        {
            std::vector<uint32_t> s0{any};
            close(s0);
            id_of(s0);
        }
        std::vector<uint32_t> moved;
        for (size_t s = 0; s < sets.size(); ++s) {
            for (uint32_t c = 0; c < C; ++c) {
                moved.clear();
                if (starts_with && sets[s].size() == 1 && sets[s][0] == accept) moved.push_back(accept);  // absorbing
                else if (c < class_rep.size())
                    for (uint32_t q : sets[s]) {
                        const uint32_t l = nfa.label[q];
                        if (l == kNoLabel) continue;
                        if (l == kAny || (*members[l])[class_rep[c]]) moved.push_back(nfa.to[q]);
                    }
                else moved.push_back(any);
                std::sort(moved.begin(), moved.end());
                moved.erase(std::unique(moved.begin(), moved.end()), moved.end());
                close(moved);
                next.push_back(uint16_t(id_of(moved)));
            }
        }
        // accepting states last: the kernel's test is one comparison
        const uint32_t S = uint32_t(sets.size());
        std::vector<uint32_t> renum(S);
        uint32_t n_rej = 0;
        std::vector<uint8_t> acc(S);
        for (uint32_t s = 0; s < S; ++s) {
            acc[s] = std::binary_search(sets[s].begin(), sets[s].end(), accept);
            n_rej += !acc[s];
        }
        uint32_t r = 0, a = n_rej;
        for (uint32_t s = 0; s < S; ++s) renum[s] = acc[s] ? a++ : r++;
        dfa.n_states = S;
        dfa.n_classes = C;
        dfa.first_accept = n_rej;
        dfa.start = renum[0];
        dfa.next.resize(size_t(S) * C);
        for (uint32_t s = 0; s < S; ++s)
            for (uint32_t c = 0; c < C; ++c) dfa.next[size_t(renum[s]) * C + c] = uint16_t(renum[next[size_t(s) * C + c]]);
        out.device = true;
    } catch (const Decline& d) {
        out.device = false;
        out.reason = d.why;
        out.dfa = Dfa{};
    }
    return out;
}

bool accepts(const Dfa& dfa, const std::vector<uint32_t>& alphabet, const uint32_t* cps, size_t n) {
    uint32_t s = dfa.start;
    for (size_t i = 0; i < n; ++i) {
        auto it = std::lower_bound(alphabet.begin(), alphabet.end(), cps[i]);
        if (it == alphabet.end() || *it != cps[i]) return false;
        s = dfa.next[size_t(s) * dfa.n_classes + dfa.cls[size_t(it - alphabet.begin())]];
    }
    return s >= dfa.first_accept;
}

}  // namespace vqregex
