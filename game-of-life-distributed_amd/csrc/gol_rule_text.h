// gol_rule_text.h — the spelling of a Life-like rule (golhip_rule_parse,
// golhip_rule_format, the "rule =" field of an RLE header).  Plain C++17 with
// no device header: the engine, the run layer and a stand-alone test program
// include the same code.
//
// A rule is two 9-bit masks (gol_rule_bits.h): bit n of birth / survive for n
// alive neighbours of 8.  Accepted: "B<digits>/S<digits>" in either letter
// case, either half possibly empty ("B2/S"), and the legacy "<survive
// digits>/<birth digits>" ("23/3"); white space around it; digits 0..8 in any
// order, none repeated.  The canonical form is "B36/S23", digits ascending.
#pragma once
#include <cstdint>
#include <string>

namespace golrule {

constexpr uint32_t kMaskAll = 0x1FF;
constexpr uint32_t kConwayBirth = 0x008, kConwaySurvive = 0x00C;

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

inline std::string format(uint32_t birth, uint32_t survive) {
    std::string s = "B";
    for (int n = 0; n < 9; ++n)
        if ((birth >> n) & 1u) s.push_back((char)('0' + n));
    s += "/S";
    for (int n = 0; n < 9; ++n)
        if ((survive >> n) & 1u) s.push_back((char)('0' + n));
    return s;
}

// False with *why naming the fault (the rule's text included).
inline bool parse(const char *text, uint32_t *birth, uint32_t *survive, std::string *why) {
    std::string t(text ? text : "");
    size_t a = 0, e = t.size();
    while (a < e && is_space(t[a])) ++a;
    while (e > a && is_space(t[e - 1])) --e;
    t = t.substr(a, e - a);
    auto bad = [&](const std::string &what) {
        *why = "rule \"" + t + "\": " + what;
        return false;
    };
    if (t.empty()) return bad("empty");
    if (t.find('/') == std::string::npos) return bad("no '/' between the two halves");
    size_t p = 0;
    // one half: its digits into *mask; stops at the first other character
    auto digits = [&](uint32_t *mask, std::string *err) {
        *mask = 0;
        for (; p < t.size() && t[p] >= '0' && t[p] <= '9'; ++p) {
            const int d = t[p] - '0';
            if (d == 9) {
                *err = "digit 9 (a cell has 0..8 neighbours)";
                return false;
            }
            if ((*mask >> d) & 1u) {
                *err = std::string("digit ") + t[p] + " repeated";
                return false;
            }
            *mask |= 1u << d;
        }
        return true;
    };
    // what may follow the second half: nothing
    auto tail = [&]() -> std::string {
        if (p == t.size()) return "";
        if (t[p] == '/') return "a third field (Generations rules B/S/C are not supported)";
        return std::string("character '") + t[p] + "' (only outer-totalistic B/S rules are supported)";
    };
    std::string err;
    uint32_t first = 0, second = 0;
    const bool letters = t[0] == 'B' || t[0] == 'b';
    if (letters) ++p;
    else if (!((t[0] >= '0' && t[0] <= '9') || t[0] == '/'))
        return bad(std::string("character '") + t[0] + "' (expected B<digits>/S<digits> or <survive>/<birth>)");
    if (!digits(&first, &err)) return bad(err);
    if (p == t.size()) return bad("no '/' between the two halves");
    if (t[p] != '/')
        return bad(std::string("character '") + t[p] + "' (only outer-totalistic B/S rules are supported)");
    ++p;
    if (letters) {
        if (p == t.size() || (t[p] != 'S' && t[p] != 's')) return bad("no S after the '/'");
        ++p;
    }
    if (!digits(&second, &err)) return bad(err);
    if (const std::string s = tail(); !s.empty()) return bad(s);
    *birth = letters ? first : second;
    *survive = letters ? second : first;
    return true;
}

// Golly's bounded-grid suffix: "<rule>:T<w>,<h>" is a torus, "<rule>:P<w>,<h>"
// a plane whose outside is dead for ever (the letter in either case, w and h
// in 1 .. 2^31 - 1; Golly's 0, an infinite dimension, is refused).
constexpr int kTorus = 0, kPlane = 1;

// parse() with an optional suffix.  Without one: kTorus and bounds 0.
inline bool parse_ex(const char *text, uint32_t *birth, uint32_t *survive, int *topology, int *bw, int *bh,
                     std::string *why) {
    std::string t(text ? text : "");
    size_t a = 0, e = t.size();
    while (a < e && is_space(t[a])) ++a;
    while (e > a && is_space(t[e - 1])) --e;
    t = t.substr(a, e - a);
    *topology = kTorus;
    *bw = *bh = 0;
    const size_t colon = t.find(':');
    if (colon == std::string::npos) return parse(t.c_str(), birth, survive, why);
    auto bad = [&](const std::string &what) {
        *why = "rule \"" + t + "\": " + what;
        return false;
    };
    const std::string head = t.substr(0, colon);
    if (!parse(head.c_str(), birth, survive, why)) {
        // the rule's own fault, under the whole text's name
        const std::string own = "rule \"" + head + "\": ";
        return bad(why->compare(0, own.size(), own) == 0 ? why->substr(own.size()) : *why);
    }
    size_t p = colon + 1;
    if (p == t.size()) return bad("nothing after the ':' (expected T<w>,<h> or P<w>,<h>)");
    const char c = t[p++];
    if (c == 'T' || c == 't') *topology = kTorus;
    else if (c == 'P' || c == 'p') *topology = kPlane;
    else return bad(std::string("topology '") + c + "' (only the torus T<w>,<h> and the plane P<w>,<h> are supported)");
    int bound[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        const char *name = k == 0 ? "width" : "height";
        if (k == 1) {
            if (p == t.size() || t[p] != ',') return bad("no ',' and height after the width (an infinite dimension is not supported)");
            ++p;
        }
        const size_t d0 = p;
        uint64_t v = 0;
        for (; p < t.size() && t[p] >= '0' && t[p] <= '9'; ++p) {
            v = v * 10 + (uint64_t)(t[p] - '0');
            if (v > 0x7FFFFFFFull) return bad(std::string("bounded ") + name + " above 2^31 - 1");
        }
        if (p == d0) return bad(std::string("no ") + name + " after the topology letter");
        if (v == 0) return bad(std::string("bounded ") + name + " 0 (an infinite dimension is not supported)");
        bound[k] = (int)v;
    }
    if (p != t.size()) return bad(std::string("character '") + t[p] + "' after the bounds");
    *bw = bound[0];
    *bh = bound[1];
    return true;
}

// The inverse; with the torus and no bounds, format()'s text.
inline std::string format_ex(uint32_t birth, uint32_t survive, int topology, int bw, int bh) {
    std::string s = format(birth, survive);
    if (bw > 0 && bh > 0)
        s += std::string(topology == kPlane ? ":P" : ":T") + std::to_string(bw) + "," + std::to_string(bh);
    return s;
}

// The rule field with a bounded-grid suffix cut off (a pattern file's bounds
// are not the board's): the text up to the first ':'.
inline std::string strip_bounds(const std::string &text) { return text.substr(0, text.find(':')); }

}  // namespace golrule
