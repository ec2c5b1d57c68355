// gol_pattern_file.h — pattern files for golhip_stamp_file:
// the run-length encoded format Life programs exchange (RLE) and the PGM
// image of gol_image_file.h, told apart by the file's first bytes.  Plain
// C++17 with no device header, so that golhip_pattern_info, the engine and a
// stand-alone test program include the same code.
//
// RLE: lines that start with '#' are skipped; the header line is
// "x = m, y = n[, rule = r]"; the body is runs <count><tag> with the tags b
// (dead), o (alive), $ (end of row) and ! (end of pattern), a missing count
// meaning 1.  White space, line breaks included, may stand anywhere between
// the body's characters, inside a run count too.  Trailing dead cells of a
// row and trailing rows may be left out.  Without a RuleMode only Conway's
// rule is accepted: B3/S23 in either letter case, 23/3, or no rule at all; a
// RuleMode accepts one other rule instead, or reports whichever the file names.
// A pattern comes out as canonical bit words: ceil(width / 32) uint32 a row,
// cell (y, x) = bit x % 32 of word x / 32, padding bits zero.
//
// RleWriter is the way back (golhip_pattern_write, golhip_save_rle; DESIGN.md
// §5.22): canonical rows in order, in as many chunks as the caller likes, to
// "<path>.tmp", renamed over <path> by commit().  It writes Golly's extended
// header "#CXRLE Pos=x,y Gen=t" (a '#' line to the parser above), the header
// line with golrule::format's spelling of the rule, and the body in lines of
// at most 70 characters: counts of 1, trailing dead cells of a row and
// trailing dead rows left out, '!' at the end.  A pattern with no alive cell
// is the header and "!".
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gol_image_file.h"
#include "gol_rule_text.h"

namespace golpat {

constexpr int kFormatRle = 0, kFormatPgm = 1;

// What a file's "rule =" field is held against: kAccept, the rule (birth,
// survive) or none; kReport, any rule golrule::parse takes.  Either way the
// file's rule comes back in (found_birth, found_survive), Conway's where it
// names none (a PGM never does).
struct RuleMode {
    enum Kind { kAccept, kReport } kind = kReport;
    uint32_t birth = golrule::kConwayBirth, survive = golrule::kConwaySurvive;
    uint32_t found_birth = golrule::kConwayBirth, found_survive = golrule::kConwaySurvive;
};

struct Info {
    int64_t width = 0, height = 0;
    uint64_t alive = 0;
    int format = kFormatRle;
    uint64_t words() const { return (uint64_t)height * (uint64_t)((width + 31) / 32); }
};

inline bool is_pgm(const unsigned char *bytes, size_t have) { return have >= 2 && bytes[0] == 'P' && bytes[1] == '5'; }

// The header of RLE text: skips '#' lines and blank lines, reads "x = m, y = n
// [, rule = r]", checks size and rule.  *body: offset of the first body byte.
inline bool rle_header(const char *t, size_t n, Info *info, size_t *body, std::string *why, RuleMode *rm = nullptr) {
    size_t pos = 0;
    auto line_end = [&](size_t p) {
        while (p < n && t[p] != '\n') ++p;
        return p;
    };
    for (;;) {
        while (pos < n && golimg::is_space((unsigned char)t[pos])) ++pos;
        if (pos < n && t[pos] == '#') {
            pos = line_end(pos);
            continue;
        }
        break;
    }
    const size_t end = line_end(pos);
    std::string line;  // the header line without white space
    for (size_t i = pos; i < end; ++i)
        if (!golimg::is_space((unsigned char)t[i])) line.push_back(t[i]);
    // x=<m>,y=<n>[,rule=<r>]
    auto number = [&](size_t &p, long long *v) {
        size_t q = p;
        unsigned long long acc = 0;
        bool neg = false;
        if (q < line.size() && line[q] == '-') neg = true, ++q;
        const size_t first = q;
        while (q < line.size() && std::isdigit((unsigned char)line[q])) {
            if (acc < (1ull << 40)) acc = acc * 10 + (unsigned)(line[q] - '0');  // (saturates far above any valid size)
            ++q;
        }
        if (q == first) return false;
        *v = neg ? -(long long)acc : (long long)acc;
        p = q;
        return true;
    };
    long long w = 0, h = 0;
    size_t p = 0;
    bool ok = line.compare(0, 2, "x=") == 0;
    if (ok) p = 2, ok = number(p, &w);
    if (ok) ok = line.compare(p, 3, ",y=") == 0;
    if (ok) p += 3, ok = number(p, &h);
    std::string rule;
    if (ok && p < line.size()) {
        ok = line.compare(p, 6, ",rule=") == 0;
        if (ok) rule = line.substr(p + 6);
    }
    if (!ok) {
        *why = "RLE: no header line \"x = m, y = n[, rule = r]\"";
        return false;
    }
    // a bounded-grid suffix (":P40,30", ":T100,7") is checked and dropped: a pattern file's bounds are not the board's
    if (rule.find(':') != std::string::npos) {
        std::string perr;
        uint32_t b = 0, s = 0;
        int topo = 0, bw = 0, bh = 0;
        if (!golrule::parse_ex(rule.c_str(), &b, &s, &topo, &bw, &bh, &perr)) {
            *why = "RLE: " + perr;
            return false;
        }
        rule = golrule::strip_bounds(rule);
    }
    if (!rule.empty() && rm) {
        std::string perr;
        if (!golrule::parse(rule.c_str(), &rm->found_birth, &rm->found_survive, &perr)) {
            *why = "RLE: " + perr;
            return false;
        }
        if (rm->kind == RuleMode::kAccept && (rm->found_birth != rm->birth || rm->found_survive != rm->survive)) {
            *why = "RLE: rule " + golrule::format(rm->found_birth, rm->found_survive) + " is not the board's " +
                   golrule::format(rm->birth, rm->survive);
            return false;
        }
    } else if (!rule.empty()) {
        std::string up;
        for (char c : rule) up.push_back((char)std::toupper((unsigned char)c));
        if (up != "B3/S23" && up != "23/3") {
            *why = "RLE: rule " + rule + " is not Conway's B3/S23";
            return false;
        }
    }
    if (w < 1 || w > INT32_MAX || h < 1 || h > INT32_MAX) {
        *why = "RLE: size " + std::to_string(w) + " x " + std::to_string(h) + " outside 1 .. 2^31 - 1";
        return false;
    }
    info->width = w;
    info->height = h;
    info->alive = 0;
    info->format = kFormatRle;
    *body = end < n ? end + 1 : n;
    return true;
}

// The body from offset `body` on, in one pass: run(y, x, len) for every run of
// alive cells, info->alive their sum.  Nothing is allocated.
template <typename Run>
inline bool rle_body(const char *t, size_t n, size_t body, Info *info, std::string *why, Run &&run) {
    const int64_t W = info->width, H = info->height;
    int64_t x = 0, y = 0, count = 0;
    bool counted = false;
    uint64_t alive = 0;
    for (size_t i = body; i < n; ++i) {
        const unsigned char c = (unsigned char)t[i];
        if (golimg::is_space(c)) continue;
        if (std::isdigit(c)) {
            count = count * 10 + (c - '0');
            counted = true;
            if (count > INT32_MAX) {
                *why = "RLE: a run leaves the " + std::to_string(W) + " x " + std::to_string(H) + " box (count past 2^31 - 1)";
                return false;
            }
            continue;
        }
        const int64_t k = counted ? count : 1;
        count = 0;
        counted = false;
        if (c == '!') {
            info->alive = alive;
            return true;
        }
        if (c == '$') {
            y += k;
            x = 0;
            if (y > H) y = H;  // (rows past the box hold no run: the next b or o reports it)
            continue;
        }
        if (c != 'b' && c != 'o') {
            *why = std::string("RLE: unknown character '") + (char)c + "' in the body";
            return false;
        }
        if (y >= H || x + k > W) {
            *why = "RLE: a run leaves the " + std::to_string(W) + " x " + std::to_string(H) + " box (row " +
                   std::to_string(y) + ", columns " + std::to_string(x) + " .. " + std::to_string(x + k) + ")";
            return false;
        }
        if (c == 'o' && k > 0) {
            run(y, x, k);
            alive += (uint64_t)k;
        }
        x += k;
    }
    *why = "RLE: no '!' before the end of the file";
    return false;
}

// Sets the bits [x, x + len) of row y of canonical words (ww a row).
inline void set_run(uint32_t *words, int64_t ww, int64_t y, int64_t x, int64_t len) {
    uint32_t *row = words + y * ww;
    while (len > 0) {
        const int64_t b = x & 31, k = std::min<int64_t>(32 - b, len);
        row[x >> 5] |= (k == 32 ? ~0u : ((1u << k) - 1u)) << b;
        x += k;
        len -= k;
    }
}

// The whole of a file (an RLE file's size goes with its runs, not with x * y).
inline bool slurp(const char *path, std::string *out, std::string *why) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) {
        *why = std::string("open ") + path + ": no such file or directory";
        return false;
    }
    char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, got);
    std::fclose(f);
    return true;
}

// A pattern file: its size and alive count (`words` null), or its cells too,
// into `words` of cap_words words (zeroed here).  0: fine; 1: *why holds the
// message of the check that failed; 2: cap_words is too small (info->width and
// height are set: info->words() are needed).  The size is checked against
// cap_words before anything is read into `words`, and `fits` (nullable) may
// refuse a size first (a pattern larger than the board it is meant for).
template <typename Fits>
inline int read(const char *path, uint32_t *words, uint64_t cap_words, Info *info, std::string *why, Fits &&fits,
                RuleMode *rm = nullptr) {
    unsigned char magic[2] = {0, 0};
    {
        std::FILE *f = std::fopen(path, "rb");
        if (!f) {
            *why = std::string("open ") + path + ": no such file or directory";
            return 1;
        }
        const size_t got = std::fread(magic, 1, 2, f);
        std::fclose(f);
        if (got < 2) magic[0] = 0;
    }
    if (is_pgm(magic, 2)) {
        golimg::Info fi;
        if (!golimg::read_info(path, 0, 0, &fi, why)) return 1;
        info->width = fi.width;
        info->height = fi.height;
        info->alive = 0;
        info->format = kFormatPgm;
        if (!fits(*info, why)) return 1;
        if (words && info->words() > cap_words) return 2;
        const int64_t ww = (fi.width + 31) / 32;
        if (words) std::memset(words, 0, (size_t)info->words() * 4);
        std::FILE *f = std::fopen(path, "rb");
        if (!f || std::fseek(f, (long)fi.header_bytes, SEEK_SET) != 0) {
            if (f) std::fclose(f);
            *why = std::string("open ") + path + ": no such file or directory";
            return 1;
        }
        std::vector<unsigned char> row((size_t)std::min<int64_t>(fi.width, 1 << 16));  // a row travels in pieces
        for (int64_t y = 0; y < fi.height; ++y)
            for (int64_t x0 = 0; x0 < fi.width; x0 += (int64_t)row.size()) {
                const size_t want = (size_t)std::min<int64_t>((int64_t)row.size(), fi.width - x0);
                if (std::fread(row.data(), 1, want, f) != want) {
                    std::fclose(f);
                    *why = std::string("short raster in ") + path;
                    return 1;
                }
                for (size_t i = 0; i < want; ++i)
                    if (row[i] == 255) {
                        ++info->alive;
                        if (words) words[y * ww + ((x0 + (int64_t)i) >> 5)] |= 1u << ((x0 + (int64_t)i) & 31);
                    }
            }
        std::fclose(f);
        return 0;
    }
    std::string text;
    if (!slurp(path, &text, why)) return 1;
    size_t body = 0;
    if (!rle_header(text.data(), text.size(), info, &body, why, rm)) return 1;
    if (!fits(*info, why)) return 1;
    if (!words) return rle_body(text.data(), text.size(), body, info, why, [](int64_t, int64_t, int64_t) {}) ? 0 : 1;
    if (info->words() > cap_words) return 2;
    std::memset(words, 0, (size_t)info->words() * 4);
    const int64_t ww = (info->width + 31) / 32;
    return rle_body(text.data(), text.size(), body, info, why,
                    [&](int64_t y, int64_t x, int64_t len) { set_run(words, ww, y, x, len); })
               ? 0
               : 1;
}

inline int read(const char *path, uint32_t *words, uint64_t cap_words, Info *info, std::string *why) {
    return read(path, words, cap_words, info, why, [](const Info &, std::string *) { return true; });
}

class RleWriter {
  public:
    RleWriter() = default;
    RleWriter(const RleWriter &) = delete;
    RleWriter &operator=(const RleWriter &) = delete;
    ~RleWriter() { abandon(); }

    // Opens <path>.tmp and writes the two header lines.  False with *why set; no file is left then.
    // plane_w, plane_h > 0: the rule carries the bounded-plane suffix ":P<plane_w>,<plane_h>".
    bool open(const char *path, int64_t pw, int64_t ph, uint32_t birth, uint32_t survive, int64_t x0, int64_t y0,
              int64_t turn, std::string *why, int plane_w = 0, int plane_h = 0) {
        path_ = path;
        tmp_ = path_ + ".tmp";
        pw_ = pw;
        ph_ = ph;
        pww_ = (pw + 31) / 32;
        fd_ = ::open(tmp_.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
        if (fd_ < 0) {
            *why = "open " + tmp_ + ": " + std::strerror(errno);
            return false;
        }
        out_ = "#CXRLE Pos=" + std::to_string(x0) + "," + std::to_string(y0) + " Gen=" + std::to_string(turn) + "\n";
        out_ += "x = " + std::to_string(pw) + ", y = " + std::to_string(ph) + ", rule = " +
                golrule::format_ex(birth, survive, golrule::kPlane, plane_w, plane_h) + "\n";
        return true;
    }

    // The next nrows rows of the pattern (canonical words, ceil(pw / 32) a row; padding bits are not looked at).
    bool feed(const uint32_t *words, int64_t nrows, std::string *why) {
        for (int64_t r = 0; r < nrows; ++r, ++row_) {
            if (row_ >= ph_) {
                *why = "RLE: more rows than the header's " + std::to_string(ph_);
                return fail_(why, nullptr);
            }
            const uint32_t *w = words + r * pww_;
            if (row_ > 0) ++dollars_;  // (a run of empty rows is carried, over chunks too, until a cell follows)
            int64_t x = 0;             // the end of the row's last alive run
            for (;;) {
                const int64_t s = next_(w, x, true);
                if (s >= pw_) break;
                const int64_t e = next_(w, s, false);
                if (dollars_) token_(dollars_, '$');
                dollars_ = 0;
                if (s > x) token_(s - x, 'b');
                token_(e - s, 'o');
                alive_ += (uint64_t)(e - s);
                x = e;
            }
            if (out_.size() >= (1u << 16) && !flush_(why)) return false;
        }
        return true;
    }

    // '!', fsync, rename over the path.  False with *why set; the .tmp file is gone then.
    bool commit(std::string *why) {
        if (fd_ < 0) {
            *why = "RLE: no file open";
            return false;
        }
        token_(1, '!');
        out_ += line_ + "\n";
        line_.clear();
        if (!flush_(why)) return false;
        if (::fsync(fd_) != 0) return fail_(why, "fsync ");
        if (::close(fd_) != 0) {
            fd_ = -1;
            ::unlink(tmp_.c_str());
            *why = "close " + tmp_ + ": " + std::strerror(errno);
            return false;
        }
        fd_ = -1;
        if (::rename(tmp_.c_str(), path_.c_str()) != 0) {
            *why = "rename " + tmp_ + ": " + std::strerror(errno);
            ::unlink(tmp_.c_str());
            return false;
        }
        return true;
    }

    // Closes and removes the .tmp file of a pattern that is not committed.
    void abandon() {
        if (fd_ < 0) return;
        ::close(fd_);
        fd_ = -1;
        ::unlink(tmp_.c_str());
    }

    uint64_t alive() const { return alive_; }

  private:
    // The first column >= from of the row whose cell is `alive` (or not); pw_ where there is none.
    int64_t next_(const uint32_t *w, int64_t from, bool alive) const {
        for (int64_t q = from >> 5; from < pw_; ++q, from = 32 * q) {
            uint32_t v = alive ? w[q] : ~w[q];
            v &= ~0u << (from & 31);
            if (v) return std::min<int64_t>(32 * q + __builtin_ctz(v), pw_);
        }
        return pw_;
    }
    void token_(int64_t count, char tag) {
        std::string t = count == 1 ? std::string() : std::to_string(count);
        t.push_back(tag);
        if (line_.size() + t.size() > 70) {
            out_ += line_ + "\n";
            line_.clear();
        }
        line_ += t;
    }
    bool flush_(std::string *why) {
        size_t done = 0;
        while (done < out_.size()) {
            const ssize_t k = ::write(fd_, out_.data() + done, out_.size() - done);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) return fail_(why, "write ");
            done += (size_t)k;
        }
        out_.clear();
        return true;
    }
    bool fail_(std::string *why, const char *call) {
        if (call) *why = call + tmp_ + ": " + std::strerror(errno);
        abandon();
        return false;
    }

    std::string path_, tmp_, out_, line_;
    int fd_ = -1;
    int64_t pw_ = 0, ph_ = 0, pww_ = 0, row_ = 0, dollars_ = 0;
    uint64_t alive_ = 0;
};

}  // namespace golpat
