// golhip_stamp.cpp — patterns: an empty board, and a
// rectangle of cells stamped anywhere on the torus at the turn the board is
// at, on the device and in the layout the board is stepped in (K10,
// gol_stamp.hip).  One handle or a group of row strips; the file layer is
// gol_pattern_file.h.
#include "golhip_impl.h"

#include "gol_pattern_file.h"

namespace gh GOLHIP_HIDDEN {

namespace {

int stamp_check(golhip_t h, const uint32_t *words, int32_t pw, int32_t ph, int32_t x0, int32_t y0, int32_t op) {
    if (!words) return fail(GOLHIP_EINVAL, "words is null");
    if (!h->loaded) return fail(GOLHIP_EINVAL, "no board loaded");
    if (op < GOLHIP_STAMP_COPY || op > GOLHIP_STAMP_CLEAR) return fail(GOLHIP_EINVAL, "unknown stamp op %d", op);
    if (pw < 1 || pw > h->W || ph < 1 || ph > h->H)
        return fail(GOLHIP_EINVAL, "pattern %d x %d does not fit the %d x %d board in one lap", pw, ph, h->W, h->H);
    if (x0 < 0 || x0 >= h->W || y0 < 0 || y0 >= h->H)
        return fail(GOLHIP_EINVAL, "stamp corner (%d, %d) not on the %d x %d board", x0, y0, h->W, h->H);
    return GOLHIP_OK;
}

// The stamp of one handle with h->mu held and the arguments checked: the rows
// of the pattern that fall on rows this handle owns (at most two intervals of
// torus rows: the pattern may cross the y seam), each staged in device scratch
// and merged by one launch a column segment.  Synchronises the stream.
int stamp_locked(golhip_t h, const uint32_t *words, int32_t pw, int32_t ph, int32_t x0, int32_t y0, int32_t op) {
    if (int rc = set_dev(h)) return rc;
    const int64_t pww = (pw + 31) / 32;
    // pattern rows [r0, r1) lie on the torus rows [t0, t0 + r1 - r0), no seam inside
    const int64_t above = std::min<int64_t>(ph, (int64_t)h->H - y0);
    const int64_t part[2][3] = {{0, above, y0}, {above, ph, 0}};
    // column segments: [x0, W) takes pattern columns from 0, [0, x0 + pw - W) the rest
    const int sw0 = std::min<int64_t>(pw, (int64_t)h->W - x0);
    const int seg[2][3] = {{x0, 0, sw0}, {0, sw0, pw - sw0}};
    bool wrote = false;
    for (const auto &p : part) {
        // the part's torus rows that this handle owns
        const int64_t lo = std::max<int64_t>(p[2], h->row0), hi = std::min<int64_t>(p[2] + p[1] - p[0], (int64_t)h->row0 + h->rows);
        if (lo >= hi) continue;
        const int64_t nr = hi - lo, pr = p[0] + (lo - p[2]);
        if (int rc = h->d_stage.ensure(h, nr * pww * 4)) return rc;
        uint32_t *d_pat = reinterpret_cast<uint32_t *>(h->d_stage.p);
        HIP_OR_FAIL(hipMemcpyAsync(d_pat, words + pr * pww, (size_t)(nr * pww) * 4, hipMemcpyHostToDevice, h->stream));
        for (const auto &s : seg) {
            if (s[2] <= 0) continue;
            golk::StampArgs a{};
            a.rows = h->cur_rows();
            a.pat = d_pat;
            a.row = lo - h->row0;
            a.nr = nr;
            a.Ww = h->Ww;
            a.pww = (int)pww;
            a.dx = s[0];
            a.sx = s[1];
            a.sw = s[2];
            a.op = op;
            HIP_OR_FAIL(golk::launch_stamp(a, h->il, h->stream));
        }
        // (the scratch is reused by the next part: its copy queues behind these launches on the stream)
        wrote = true;
    }
    if (int rc = sync_stream(h)) return rc;
    if (wrote) {
        h->alive_turn = -1;
        h->flips_valid = false;
    }
    return GOLHIP_OK;
}

void fill_info(const golpat::Info &pi, golhip_pattern_info_t *info) {
    memset(info, 0, sizeof *info);
    info->width = (int32_t)pi.width;
    info->height = (int32_t)pi.height;
    info->alive = pi.alive;
    info->format = pi.format;
}

}  // namespace

}  // namespace gh

using namespace gh;

extern "C" {

int golhip_clear(golhip_t h) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    HIP_OR_FAIL(hipMemsetAsync(h->cur_rows(), 0, (size_t)h->local_words() * 4, h->stream));
    if (int rc = loaded_canonical(h)) return rc;
    if (int rc_ = sync_stream(h)) return rc_;
    h->turns = 0;
    h->alive_turn = -1;
    h->flips_valid = false;
    return GOLHIP_OK;
}

int golhip_stamp_bits(golhip_t h, const uint32_t *words, int32_t pw, int32_t ph, int32_t x0, int32_t y0, int32_t op) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = stamp_check(h, words, pw, ph, x0, y0, op)) return rc;
    return stamp_locked(h, words, pw, ph, x0, y0, op);
}

int golhip_group_stamp_bits(golhip_t *hs, int32_t n, const uint32_t *words, int32_t pw, int32_t ph, int32_t x0,
                            int32_t y0, int32_t op) {
    if (int rc = group_check(hs, n)) return rc;
    if (int rc = stamp_check(hs[0], words, pw, ph, x0, y0, op)) return rc;
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    for (int i = 0; i < n; ++i)
        if (int rc = stamp_locked(hs[i], words, pw, ph, x0, y0, op)) return rc;
    return GOLHIP_OK;
}

int golhip_pattern_info(const char *path, golhip_pattern_info_t *info) {
    if (!path || !info) return fail(GOLHIP_EINVAL, "null argument");
    golpat::Info pi;
    std::string why;
    if (golpat::read(path, nullptr, 0, &pi, &why)) return fail(GOLHIP_EINVAL, "%s", why.c_str());
    fill_info(pi, info);
    return GOLHIP_OK;
}

int golhip_pattern_read(const char *path, uint32_t *words, uint64_t cap_words, golhip_pattern_info_t *info) {
    if (!path || !info || !words) return fail(GOLHIP_EINVAL, "null argument");
    golpat::Info pi;
    std::string why;
    const int r = golpat::read(path, words, cap_words, &pi, &why);
    if (r == 1) return fail(GOLHIP_EINVAL, "%s", why.c_str());
    fill_info(pi, info);
    if (r == 2)
        return fail(GOLHIP_ERANGE, "pattern %s needs %llu words, the buffer holds %llu", path, (unsigned long long)pi.words(),
                    (unsigned long long)cap_words);
    return GOLHIP_OK;
}

int golhip_pattern_rule(const char *path, uint32_t *birth, uint32_t *survive) {
    if (!path || !birth || !survive) return fail(GOLHIP_EINVAL, "null argument");
    golpat::Info pi;
    golpat::RuleMode mode;  // kReport
    std::string why;
    if (golpat::read(path, nullptr, 0, &pi, &why, [](const golpat::Info &, std::string *) { return true; }, &mode))
        return fail(GOLHIP_EINVAL, "%s", why.c_str());
    *birth = mode.found_birth;
    *survive = mode.found_survive;
    return GOLHIP_OK;
}

int golhip_stamp_file(golhip_t *hs, int32_t n, const char *path, int32_t x0, int32_t y0, int32_t op,
                      golhip_pattern_info_t *info) {
    if (!path) return fail(GOLHIP_EINVAL, "path is null");
    if (int rc = group_check(hs, n)) return rc;
    const int W = hs[0]->W, H = hs[0]->H;
    // the size is checked against the board before the pattern's words are allocated
    auto fits = [&](const golpat::Info &pi, std::string *why) {
        if (pi.width <= W && pi.height <= H) return true;
        *why = "pattern " + std::string(path) + " is " + std::to_string(pi.width) + " x " + std::to_string(pi.height) +
               ": it does not fit the " + std::to_string(W) + " x " + std::to_string(H) + " board in one lap";
        return false;
    };
    golpat::Info pi;
    std::string why;
    // a Conway board takes what it always took; a board with another rule takes a file of that rule, or of none
    golpat::RuleMode mode;
    mode.kind = golpat::RuleMode::kAccept;
    mode.birth = hs[0]->birth;
    mode.survive = hs[0]->survive;
    golpat::RuleMode *rm = hs[0]->conway() ? nullptr : &mode;
    if (golpat::read(path, nullptr, 0, &pi, &why, fits, rm)) return fail(GOLHIP_EINVAL, "%s", why.c_str());
    std::vector<uint32_t> words((size_t)pi.words());
    if (golpat::read(path, words.data(), words.size(), &pi, &why, fits, rm)) return fail(GOLHIP_EINVAL, "%s", why.c_str());
    if (int rc = golhip_group_stamp_bits(hs, n, words.data(), (int32_t)pi.width, (int32_t)pi.height, x0, y0, op)) return rc;
    if (info) fill_info(pi, info);
    return GOLHIP_OK;
}

}  // extern "C"
