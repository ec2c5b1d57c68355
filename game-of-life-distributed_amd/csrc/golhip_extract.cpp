// golhip_extract.cpp — saving patterns, the read half of
// golhip_stamp.cpp: any rectangle of the torus as canonical bit words (K12,
// gol_extract.hip), the alive box from the occupancy bitmaps (K13; gol_box.h),
// and RLE files of either (RleWriter, gol_pattern_file.h).  One handle or a
// group of row strips.  Observers: nothing here writes a board, a turn, a kept
// count or a kept flip list.
#include "golhip_impl.h"

#include "gol_box.h"
#include "gol_pattern_file.h"

namespace gh GOLHIP_HIDDEN {

namespace {

constexpr int64_t kChunkBytes = 16ll << 20;  // device scratch of one extract round; golhip_save_rle's default chunk

int extract_check(golhip_t h, const uint32_t *words, int32_t x0, int32_t y0, int32_t pw, int32_t ph, uint64_t cap_words) {
    if (!words) return fail(GOLHIP_EINVAL, "words is null");
    if (!h->loaded) return fail(GOLHIP_EINVAL, "no board loaded");
    if (pw < 1 || pw > h->W || ph < 1 || ph > h->H)
        return fail(GOLHIP_EINVAL, "rectangle %d x %d does not fit the %d x %d board in one lap", pw, ph, h->W, h->H);
    if (x0 < 0 || x0 >= h->W || y0 < 0 || y0 >= h->H)
        return fail(GOLHIP_EINVAL, "corner (%d, %d) not on the %d x %d board", x0, y0, h->W, h->H);
    const uint64_t need = (uint64_t)ph * (uint64_t)((pw + 31) / 32);
    if (cap_words < need)
        return fail(GOLHIP_ERANGE, "rectangle %d x %d needs %llu words, the buffer holds %llu", pw, ph, (unsigned long long)need,
                    (unsigned long long)cap_words);
    return GOLHIP_OK;
}

// The extract of one handle with h->mu held and the arguments checked: the rows
// of the rectangle that fall on rows this handle owns (at most two intervals
// of torus rows), each zeroed in device scratch, filled by one launch a column
// segment and copied to its place in `words`; rows the handle does not own are
// not touched.  Synchronises the stream.
int extract_locked(golhip_t h, int32_t x0, int32_t y0, int32_t pw, int32_t ph, uint32_t *words) {
    if (int rc = set_dev(h)) return rc;
    const int64_t pww = (pw + 31) / 32;
    const int64_t above = std::min<int64_t>(ph, (int64_t)h->H - y0);
    const int64_t part[2][3] = {{0, above, y0}, {above, ph, 0}};
    // column segments: [x0, W) goes to output columns from 0, [0, x0 + pw - W) behind them
    const int sw0 = (int)std::min<int64_t>(pw, (int64_t)h->W - x0);
    const int seg[2][3] = {{x0, 0, sw0}, {0, sw0, pw - sw0}};
    const int64_t round_rows = std::max<int64_t>(1, kChunkBytes / (pww * 4));
    for (const auto &p : part) {
        const int64_t lo = std::max<int64_t>(p[2], h->row0), hi = std::min<int64_t>(p[2] + p[1] - p[0], (int64_t)h->row0 + h->rows);
        for (int64_t t = lo; t < hi; t += round_rows) {
            const int64_t nr = std::min(round_rows, hi - t), pr = p[0] + (t - p[2]);
            if (int rc = h->d_stage.ensure(h, nr * pww * 4)) return rc;
            uint32_t *d_out = reinterpret_cast<uint32_t *>(h->d_stage.p);
            // (the scratch is reused by the next round: its memset queues behind this round's copy on the stream)
            HIP_OR_FAIL(hipMemsetAsync(d_out, 0, (size_t)(nr * pww) * 4, h->stream));
            for (const auto &s : seg) {
                if (s[2] <= 0) continue;
                golk::ExtractArgs a{};
                a.rows = h->cur_rows();
                a.out = d_out;
                a.row = t - h->row0;
                a.nr = nr;
                a.Ww = h->Ww;
                a.pww = (int)pww;
                a.sx = s[0];
                a.ox = s[1];
                a.sw = s[2];
                HIP_OR_FAIL(golk::launch_extract(a, h->il, h->stream));
            }
            HIP_OR_FAIL(hipMemcpyAsync(words + pr * pww, d_out, (size_t)(nr * pww) * 4, hipMemcpyDeviceToHost, h->stream));
        }
    }
    return sync_stream(h);
}

// Every strip's mutex, in group order (the order golhip_group_stamp_bits takes them in).
struct GroupLock {
    std::vector<std::unique_lock<std::mutex>> locks;
    GroupLock(golhip_t *hs, int32_t n) {
        for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    }
};

int group_extract_locked(golhip_t *hs, int32_t n, int32_t x0, int32_t y0, int32_t pw, int32_t ph, uint32_t *words) {
    for (int i = 0; i < n; ++i)
        if (int rc = extract_locked(hs[i], x0, y0, pw, ph, words)) return rc;
    return GOLHIP_OK;
}

struct Box {
    int32_t x0 = 0, y0 = 0, pw = 0, ph = 0;
};

// The alive box of the group's board, every strip's mutex held: K13 on every
// strip's own rows, the column words ORed and the row bits appended in row order.
int alive_box_locked(golhip_t *hs, int32_t n, Box *box) {
    const int W = hs[0]->W, H = hs[0]->H, Ww = hs[0]->Ww;
    std::vector<uint32_t> col((size_t)Ww, 0u), row((size_t)(((int64_t)H + 31) / 32 + 1), 0u), part;
    for (int i = 0; i < n; ++i) {
        golhip_t h = hs[i];
        if (h->rows <= 0) continue;
        if (int rc = set_dev(h)) return rc;
        const int64_t rw = ((int64_t)h->rows + 31) / 32, nw = Ww + rw;
        if (int rc = h->d_stage.ensure(h, nw * 4)) return rc;
        uint32_t *d = reinterpret_cast<uint32_t *>(h->d_stage.p);
        HIP_OR_FAIL(hipMemsetAsync(d, 0, (size_t)nw * 4, h->stream));
        HIP_OR_FAIL(golk::launch_occupancy(h->cur_rows(), h->rows, Ww, h->il, d, d + Ww, h->stream));
        part.assign((size_t)nw, 0u);
        HIP_OR_FAIL(hipMemcpyAsync(part.data(), d, (size_t)nw * 4, hipMemcpyDeviceToHost, h->stream));
        if (int rc = sync_stream(h)) return rc;
        for (int j = 0; j < Ww; ++j) col[(size_t)j] |= part[(size_t)j];
        golbox::append_bits(row.data(), h->row0, part.data() + Ww, h->rows);
    }
    // (a bounded plane has no seam: the plain min / max box)
    const bool plane = hs[0]->plane;
    const golbox::Interval ix = plane ? golbox::interval_plane(col.data(), W) : golbox::interval(col.data(), W),
                           iy = plane ? golbox::interval_plane(row.data(), H) : golbox::interval(row.data(), H);
    *box = Box{};
    if (ix.len == 0 || iy.len == 0) return GOLHIP_OK;
    box->x0 = (int32_t)ix.start;
    box->pw = (int32_t)ix.len;
    box->y0 = (int32_t)iy.start;
    box->ph = (int32_t)iy.len;
    return GOLHIP_OK;
}

}  // namespace

}  // namespace gh

using namespace gh;

extern "C" {

int golhip_extract_bits(golhip_t h, int32_t x0, int32_t y0, int32_t pw, int32_t ph, uint32_t *words, uint64_t cap_words) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = extract_check(h, words, x0, y0, pw, ph, cap_words)) return rc;
    // a strip: the rows it does not own come back zero
    if (h->rows != h->H) memset(words, 0, (size_t)ph * (size_t)((pw + 31) / 32) * 4);
    return extract_locked(h, x0, y0, pw, ph, words);
}

int golhip_group_extract_bits(golhip_t *hs, int32_t n, int32_t x0, int32_t y0, int32_t pw, int32_t ph, uint32_t *words,
                              uint64_t cap_words) {
    if (int rc = group_check(hs, n)) return rc;
    if (int rc = extract_check(hs[0], words, x0, y0, pw, ph, cap_words)) return rc;
    GroupLock g(hs, n);
    return group_extract_locked(hs, n, x0, y0, pw, ph, words);
}

int golhip_alive_box(golhip_t *hs, int32_t n, int32_t *x0, int32_t *y0, int32_t *pw, int32_t *ph) {
    if (!x0 || !y0 || !pw || !ph) return fail(GOLHIP_EINVAL, "null out");
    if (int rc = group_check(hs, n)) return rc;
    GroupLock g(hs, n);
    Box b;
    if (int rc = alive_box_locked(hs, n, &b)) return rc;
    *x0 = b.x0;
    *y0 = b.y0;
    *pw = b.pw;
    *ph = b.ph;
    return GOLHIP_OK;
}

int golhip_box_interval(const uint32_t *bits, int32_t n, int32_t *start, int32_t *len) {
    if (!bits || !start || !len) return fail(GOLHIP_EINVAL, "null argument");
    if (n < 1) return fail(GOLHIP_EINVAL, "an axis of %d positions", n);
    const golbox::Interval iv = golbox::interval(bits, n);
    *start = (int32_t)iv.start;
    *len = (int32_t)iv.len;
    return GOLHIP_OK;
}

int golhip_pattern_write(const char *path, const uint32_t *words, int32_t pw, int32_t ph, uint32_t birth, uint32_t survive,
                         int32_t x0, int32_t y0, int64_t turn) {
    if (!path || !words) return fail(GOLHIP_EINVAL, "null argument");
    if (pw < 1 || ph < 1) return fail(GOLHIP_EINVAL, "pattern %d x %d: sizes start at 1", pw, ph);
    if (birth > golrule::kMaskAll || survive > golrule::kMaskAll)
        return fail(GOLHIP_EINVAL, "rule masks 0x%x / 0x%x above 0x1FF", birth, survive);
    golpat::RleWriter w;
    std::string why;
    if (!w.open(path, pw, ph, birth, survive, x0, y0, turn, &why) || !w.feed(words, ph, &why) || !w.commit(&why))
        return fail(GOLHIP_EINVAL, "%s", why.c_str());
    return GOLHIP_OK;
}

int golhip_save_rle(golhip_t *hs, int32_t n, const char *path, int32_t x0, int32_t y0, int32_t pw, int32_t ph,
                    int32_t chunk_rows, golhip_pattern_info_t *info) {
    if (!path) return fail(GOLHIP_EINVAL, "path is null");
    if (chunk_rows < 0) return fail(GOLHIP_EINVAL, "chunk_rows %d is negative", chunk_rows);
    if (int rc = group_check(hs, n)) return rc;
    // one critical section: box, cells and turn belong to the same board
    GroupLock g(hs, n);
    if (pw == 0 && ph == 0) {
        Box b;
        if (int rc = alive_box_locked(hs, n, &b)) return rc;
        if (b.pw == 0) return fail(GOLHIP_EINVAL, "board is empty");
        x0 = b.x0;
        y0 = b.y0;
        pw = b.pw;
        ph = b.ph;
    }
    const int64_t pww = (pw + 31) / 32;
    // (checked against a buffer of exactly the size: the words are allocated below, a chunk at a time)
    uint32_t probe = 0;
    if (int rc = extract_check(hs[0], &probe, x0, y0, pw, ph, (uint64_t)ph * (uint64_t)pww)) return rc;
    const int64_t turn = hs[0]->turns.load();
    for (int i = 1; i < n; ++i)
        if (hs[i]->turns.load() != turn) return fail(GOLHIP_EINVAL, "strip %d is at turn %lld, strip 0 at %lld", i,
                                                     (long long)hs[i]->turns.load(), (long long)turn);
    const int64_t chunk = chunk_rows ? chunk_rows : std::max<int64_t>(1, kChunkBytes / (pww * 4));
    std::vector<uint32_t> words((size_t)(std::min<int64_t>(chunk, ph) * pww));
    golpat::RleWriter w;
    std::string why;
    // (a plane handle: "rule = B3/S23:P<W>,<H>", so the file reopens bounded)
    const bool plane = hs[0]->plane;
    if (!w.open(path, pw, ph, hs[0]->birth, hs[0]->survive, x0, y0, turn, &why, plane ? hs[0]->W : 0, plane ? hs[0]->H : 0))
        return fail(GOLHIP_EINVAL, "%s", why.c_str());
    for (int64_t r = 0; r < ph; r += chunk) {
        const int32_t nr = (int32_t)std::min<int64_t>(chunk, ph - r);
        // (w's destructor removes the .tmp file on every early return)
        if (int rc = group_extract_locked(hs, n, x0, (int32_t)(((int64_t)y0 + r) % hs[0]->H), pw, nr, words.data())) return rc;
        if (!w.feed(words.data(), nr, &why)) return fail(GOLHIP_EINVAL, "%s", why.c_str());
    }
    if (!w.commit(&why)) return fail(GOLHIP_EINVAL, "%s", why.c_str());
    if (info) {
        memset(info, 0, sizeof *info);
        info->width = pw;
        info->height = ph;
        info->alive = w.alive();
        info->format = golpat::kFormatRle;
    }
    return GOLHIP_OK;
}

}  // extern "C"
