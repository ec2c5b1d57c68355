// golhip_pad.cpp — the padded torus: a whole torus whose
// width is no multiple of 32 steps on the per-launch kernels (K1w / K1) as a
// Wp x H torus with ghost columns, refreshed between launches (gol_pad.hip),
// instead of one turn a launch on K1g.  The wide board is an internal handle
// of this one; the canonical board is whole again when a step returns.
// The strips of a group (golhip_group_step) do the same with one wide strip
// each, halo rows included: padded strips, the second half of this file.
#include "golhip_impl.h"

namespace gh GOLHIP_HIDDEN {

bool pad_applies(golhip_t h) {
    golk::PadPlan p;
    // (ghost columns are copies of real ones; a bounded plane has none and runs any width on K15)
    return h->W % 32 != 0 && h->torus() && !h->ringed() && !h->plane && golk::pad_plan(h->W, &p);
}

// The measured rule (profiles/widths/bench_widths.json):
// the (cells, turns a call) region where the padded path beat K1g in every
// repetition.  A call pays the pad and the unpad pass once: calls of two turns
// or more won at every size measured (100^2: 2.2x at 2 turns; 16385^2: 31x),
// one-turn calls from 1000^2 on (1.3x; 16385^2: 25x) but lost at 100^2 (0.96x,
// every repetition), so below the smallest board they won at they stay on K1g.
// Measured on Conway's kernels; a handle with another rule (K11 on the wide
// board, K11's one-turn any-width form instead of K1g) keeps it until its own
// sweep exists.
struct PadRule {
    int64_t min_cells, min_turns;
};
static constexpr PadRule kPadRule[] = {
    {0, 2},
    {1000 * 1000, 1},
};
static bool pad_auto(int64_t cells, int64_t nturns) {
    for (const PadRule &r : kPadRule)
        if (cells >= r.min_cells && nturns >= r.min_turns) return true;
    return false;
}

bool pad_wanted(golhip_t h, int64_t nturns) {
    if (nturns < 1 || h->pad_mode == 0 || !pad_applies(h)) return false;
    if (h->pad_mode == 1) return true;
    return !h->pad_nomem && pad_auto((int64_t)h->W * h->H, nturns);
}

int pad_destroy(golhip_t h) {
    if (!h->wide) return GOLHIP_OK;
    golhip *w = h->wide;
    h->wide = nullptr;
    w->d_trace = nullptr;  // the owner's
    return golhip_destroy(w);
}

// The wide board: Wp columns, the owner's rows of the torus (all of them, or
// a strip's with its halo rows), on the owner's device and stream.
static int ensure_wide(golhip_t h) {
    if (h->wide) return GOLHIP_OK;
    golk::PadPlan p;
    if (!golk::pad_plan(h->W, &p)) return fail(GOLHIP_EINVAL, "no padded torus for width %d", h->W);
    golhip *w = new golhip();
    w->W = p.Wp;
    w->H = h->H;
    w->Ww = p.Wp / 32;
    w->row0 = h->row0;
    w->rows = h->rows;
    w->strip = h->strip;
    w->device = h->device;
    w->flags = h->flags;
    w->stream = h->stream;
    w->phys_rows = (int64_t)w->rows + 2 * kHalo;
    w->cu_count = h->cu_count;
    w->dev_cu = h->dev_cu;
    // the resident kernels run many turns with no place for a refresh
    w->persistent = 0;
    w->lds_band = 0;
    // every launch pays a seam refresh, so the automatic plan keeps the deep
    // launches of one or two words per lane; "wpl" 4 on the owner still gives quads
    w->no_quads = true;
    const size_t bytes = (size_t)w->phys_rows * w->Ww * sizeof(uint32_t);
    hipError_t e = hipMalloc(&w->buf[0], bytes);
    if (e == hipSuccess) e = hipMalloc(&w->buf[1], bytes);
    if (e == hipSuccess) e = hipMemsetAsync(w->buf[0], 0, bytes, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(w->buf[1], 0, bytes, h->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)golhip_destroy(w);
        const int code = e == hipErrorOutOfMemory ? GOLHIP_ENOMEM : GOLHIP_EHIP;
        return fail(code, "padded torus %d x %d (%zu bytes x2): %s", p.Wp, h->rows, bytes, hipGetErrorString(e));
    }
    h->wide = w;
    return GOLHIP_OK;
}

// The wide board plans with the owner's settings at every step, so tests and
// A/Bs steer it through the owner.
static void take_settings(golhip_t h, golhip *w) {
    w->stream = h->stream;
    w->flags = h->flags;
    if (w->wpl_opt != h->wpl_opt || w->cu_count != h->cu_count || w->fill_skip != h->fill_skip ||
        w->paired_bands != h->paired_bands || w->birth != h->birth || w->survive != h->survive ||
        w->rule_kernel != h->rule_kernel)
        for (int &c : w->auto_rpw) c = 0;
    // the owner's rule: ghost columns are copies of real ones under any radius-1 rule, B0 included
    w->birth = h->birth;
    w->survive = h->survive;
    w->rule_kernel = h->rule_kernel;
    w->wpl_opt = h->wpl_opt;
    w->cu_count = h->cu_count;
    w->fill_skip = h->fill_skip;
    w->paired_bands = h->paired_bands;
    w->tb_depth = h->tb_depth;
    w->rows_per_wave = h->rows_per_wave;
    w->dummy_rows = h->dummy_rows;
    w->skew = h->skew;
    w->skew_young = h->skew_young;
    w->skew_hcap = h->skew_hcap;
    w->skew_prio = h->skew_prio;
    w->skew_tx = h->skew_tx;
    w->skew_half = h->skew_half;
    w->skew_pairs = h->skew_pairs;
    w->skew_interior = h->skew_interior;
    w->d_trace = h->d_trace;
}

int pad_step(golhip_t h, int64_t nturns, bool *ran) {
    *ran = false;
    if (int rc = ensure_wide(h)) {
        if (h->pad_mode == 1 || rc != GOLHIP_ENOMEM) return rc;
        h->pad_nomem = true;  // the rule: K1g from here on
        return GOLHIP_OK;
    }
    golhip *w = h->wide;
    take_settings(h, w);
    // the pad kernel writes the layout the wide board steps in
    w->il = want_il(w);
    w->loaded = true;
    golk::PadArgs a{};
    golk::pad_plan(h->W, &a.plan);
    a.canon = h->cur_rows();  // (canonical: W % 64 != 0 runs one word per lane)
    a.wide = w->cur_rows();
    a.rows = h->rows;
    a.Ww = h->Ww;
    a.Wwp = w->Ww;
    w->n = Counters{};
    HIP_OR_FAIL(golk::launch_pad(a, w->il, h->stream));
    for (int64_t left = nturns; left > 0;) {
        const int d = depth_plan(depth_cap(w, false), left).d;
        if (left != nturns) {  // (the pad pass wrote the first launch's ghosts)
            a.wide = w->cur_rows();
            HIP_OR_FAIL(golk::launch_seam(a, w->il, h->stream));
        }
        h->n.pad_launches++;
        if (int rc = launch_depth(w, d, false, false)) return rc;
        left -= d;
    }
    a.wide = w->cur_rows();
    a.alive = h->d_scalars;  // the wide board's fused count would include the ghosts
    HIP_OR_FAIL(hipMemsetAsync(h->d_scalars, 0, sizeof(unsigned long long), h->stream));
    HIP_OR_FAIL(golk::launch_unpad(a, w->il, h->stream));
    h->turns += nturns;
    h->alive_turn = h->turns;
    h->n.step_launches += w->n.step_launches;
    h->n.step_turns += w->n.step_turns;
    h->n.skew_launches += w->n.skew_launches;
    h->n.skew_half_launches += w->n.skew_half_launches;
    h->n.pair_launches += w->n.pair_launches;
    h->n.pair_turns += w->n.pair_turns;
    h->n.rule_launches += w->n.rule_launches;
    h->last_variant = w->last_variant;
    *ran = true;
    return GOLHIP_OK;
}

// ---- padded strips ------------------------------------------------------------
// Every strip of a group owns a wide strip; a group_step call pads every
// strip's own rows, runs the group's rounds over the wide strips (one deep-halo
// exchange of k d wide rows, then k launches) and unpads.  The invariant:
// every wide row a launch reads has had its ghosts rewritten from its own real
// columns since it was last written, by a launch or by an exchange.  Exchanged
// rows carry the neighbour's stale ghosts but exact real columns, so the seam
// refresh before a launch covers the halo rows that launch reads too.

// The measured rule of padded strips (profiles/strip_widths/bench_strip_widths.json,
// DESIGN.md §5.17 "Padded strips"): per measured board, the fewest turns a call
// from which mode 1 beat mode 0 in every repetition at 2, 4 and 8 strips alike
// (and at every larger n measured).  A board takes the row of the largest
// measured board that is no larger than it; boards below 100^2 take 100^2's.
//   100^2    n = 1, 2 lost (0.82-0.96x, 0.88-1.08x), 4 won (1.06-1.33x)
//   1000^2   n = 1, 2, 4 lost or tied at 4 or 8 strips (n = 4: 1.04-1.43x, not every repetition), 8 won (1.33-1.90x)
//   5000^2   n = 1 tied at 4 and 8 strips (1.02-1.05x), 2 won (1.15-2.39x)
//   10001^2  n = 1 won (1.76-3.80x); 16385^2 n = 1 won (2.77-6.95x)
// The group pays a pad and an unpad launch a strip and a call beside K1g's one
// launch a turn, so short calls of many small strips are launch-bound and lose.
static constexpr PadRule kStripPadRule[] = {
    {0, 4},
    {1000ll * 1000, 8},
    {5000ll * 5000, 2},
    {10001ll * 10001, 1},
};
static bool strip_pad_auto(int64_t cells, int64_t nturns) {
    int64_t min_turns = kStripPadRule[0].min_turns;
    for (const PadRule &r : kStripPadRule)
        if (cells >= r.min_cells) min_turns = r.min_turns;
    return nturns >= min_turns;
}

static bool pad_group_applies(golhip_t *hs, int32_t n) {
    golk::PadPlan p;
    if (hs[0]->W % 32 == 0 || hs[0]->plane || !golk::pad_plan(hs[0]->W, &p)) return false;
    for (int i = 0; i < n; ++i)
        if (hs[i]->ringed()) return false;
    return true;
}

bool pad_group_wanted(golhip_t *hs, int32_t n, int64_t nturns) {
    const int mode = hs[0]->group_pad_mode;
    if (nturns < 1 || mode == 0 || !pad_group_applies(hs, n)) return false;
    if (mode == 1) return true;
    for (int i = 0; i < n; ++i)
        if (hs[i]->group_pad_nomem) return false;
    return strip_pad_auto((int64_t)hs[0]->W * hs[0]->H, nturns);
}

static golk::PadArgs pad_args(golhip_t h) {
    golhip *w = h->wide;
    golk::PadArgs a{};
    golk::pad_plan(h->W, &a.plan);
    a.canon = h->cur_rows();
    a.wide = w->cur_rows();
    a.rows = h->rows;
    a.Ww = h->Ww;
    a.Wwp = w->Ww;
    return a;
}

int pad_seam(golhip_t h, int lo, int hi) {
    golhip *w = h->wide;
    // (the halo rows: kHalo above the strip's first row, kHalo below its last)
    if (lo < -kHalo || hi > w->rows + kHalo || lo > hi) return fail(GOLHIP_EINVAL, "seam rows [%d, %d) of %d", lo, hi, w->rows);
    golk::PadArgs a = pad_args(h);
    a.canon = nullptr;
    a.wide = w->buf[w->cur] + ((int64_t)kHalo + lo) * w->Ww;
    a.rows = hi - lo;
    HIP_OR_FAIL(golk::launch_seam(a, w->il, w->stream));
    h->n.pad_launches++;
    return GOLHIP_OK;
}

int pad_group_step(golhip_t *hs, int32_t n, int64_t nturns, hipEvent_t *ready, bool *ran) {
    *ran = false;
    for (int i = 0; i < n; ++i) {
        HIP_OR_FAIL(hipSetDevice(hs[i]->device));
        const int rc = ensure_wide(hs[i]);
        if (!rc) continue;
        if (hs[0]->group_pad_mode == 1 || rc != GOLHIP_ENOMEM) return rc;
        // the rule: every strip or none, so the whole group stays on K1g from here on
        for (int j = 0; j < n; ++j) {
            hs[j]->group_pad_nomem = true;
            HIP_OR_FAIL(hipSetDevice(hs[j]->device));
            if (int prc = pad_destroy(hs[j])) return prc;
        }
        return GOLHIP_OK;
    }
    std::vector<golhip_t> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
        golhip *h = hs[i], *w = h->wide;
        take_settings(h, w);
        w->il = want_il(w);  // the pad kernel writes the layout the wide strips step in
        w->loaded = true;
        w->n = Counters{};
        ws[i] = w;
        if (w->il != hs[0]->wide->il) return fail(GOLHIP_EINVAL, "strip %d uses another word layout", i);
    }
    for (int i = 0; i < n; ++i) {
        HIP_OR_FAIL(hipSetDevice(hs[i]->device));
        HIP_OR_FAIL(golk::launch_pad(pad_args(hs[i]), ws[i]->il, hs[i]->stream));
    }
    if (int rc = group_rounds(ws.data(), hs, n, nturns, false, ready)) return rc;
    for (int i = 0; i < n; ++i) {
        golhip *h = hs[i], *w = ws[i];
        HIP_OR_FAIL(hipSetDevice(h->device));
        golk::PadArgs a = pad_args(h);
        a.alive = h->d_scalars;  // the strip's own rows and real columns alone
        HIP_OR_FAIL(hipMemsetAsync(h->d_scalars, 0, sizeof(unsigned long long), h->stream));
        HIP_OR_FAIL(golk::launch_unpad(a, w->il, h->stream));
        h->turns += nturns;
        h->alive_turn = h->turns;
        h->n.step_launches += w->n.step_launches;
        h->n.step_turns += w->n.step_turns;
        h->n.skew_launches += w->n.skew_launches;
        h->n.skew_half_launches += w->n.skew_half_launches;
        h->n.pair_launches += w->n.pair_launches;
        h->n.pair_turns += w->n.pair_turns;
        h->n.rule_launches += w->n.rule_launches;
        h->n.halo_bytes += w->n.halo_bytes;
        h->n.halo_exchanges += w->n.halo_exchanges;
        h->last_variant = w->last_variant;
    }
    *ran = true;
    return GOLHIP_OK;
}

}  // namespace gh

using namespace gh;

extern "C" {

int golhip_set_pad_step(golhip_t h, int32_t mode) {
    if (int rc = check(h)) return rc;
    if (mode < -1 || mode > 1) return fail(GOLHIP_EINVAL, "pad step mode %d not in -1..1", mode);
    std::lock_guard<std::mutex> g(h->mu);
    if (mode == 1 && h->plane)
        return fail(GOLHIP_EINVAL, "the padded torus copies columns across the row seam: a bounded plane has none "
                                   "(golhip_set_topology) and steps any width without it");
    if (mode == 1 && !pad_applies(h))
        return fail(GOLHIP_EINVAL, "the padded torus is for a whole torus without a communicator whose width is no "
                                   "multiple of 32 (width %d, rows %d of %d)", h->W, h->rows, h->H);
    h->pad_mode = mode;
    h->pad_nomem = false;
    return GOLHIP_OK;
}

int golhip_group_set_pad_step(golhip_t *hs, int32_t n, int32_t mode) {
    if (int rc = group_check(hs, n, false)) return rc;
    if (mode < -1 || mode > 1) return fail(GOLHIP_EINVAL, "pad step mode %d not in -1..1", mode);
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    if (mode == 1 && !pad_group_applies(hs, n))
        return fail(GOLHIP_EINVAL, "padded strips are for a group without a communicator whose width is no "
                                   "multiple of 32 (width %d)", hs[0]->W);
    for (int i = 0; i < n; ++i) {
        hs[i]->group_pad_mode = mode;
        hs[i]->group_pad_nomem = false;
    }
    return GOLHIP_OK;
}

}  // extern "C"
