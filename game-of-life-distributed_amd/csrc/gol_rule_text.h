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

}  // namespace golrule
