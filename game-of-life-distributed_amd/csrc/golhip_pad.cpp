// golhip_pad.cpp — the padded torus: a whole torus whose
// width is no multiple of 32 steps on the per-launch kernels (K1w / K1) as a
// Wp x H torus with ghost columns, refreshed between launches (gol_pad.hip),
// instead of one turn a launch on K1g.  The wide board is an internal handle
// of this one; the canonical board is whole again when a step returns.
#include "golhip_impl.h"

namespace gh GOLHIP_HIDDEN {

bool pad_applies(golhip_t h) {
    golk::PadPlan p;
    return h->W % 32 != 0 && h->torus() && !h->ringed() && golk::pad_plan(h->W, &p);
}

// The measured rule (profiles/widths/bench_widths.json):
// the (cells, turns a call) region where the padded path beat K1g in every
// repetition.  A call pays the pad and the unpad pass once: calls of two turns
// or more won at every size measured (100^2: 2.2x at 2 turns; 16385^2: 31x),
// one-turn calls from 1000^2 on (1.3x; 16385^2: 25x) but lost at 100^2 (0.96x,
// every repetition), so below the smallest board they won at they stay on K1g.
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

// The wide board: Wp x H on the owner's device and stream.
static int ensure_wide(golhip_t h) {
    if (h->wide) return GOLHIP_OK;
    golk::PadPlan p;
    if (!golk::pad_plan(h->W, &p)) return fail(GOLHIP_EINVAL, "no padded torus for width %d", h->W);
    golhip *w = new golhip();
    w->W = p.Wp;
    w->H = h->H;
    w->Ww = p.Wp / 32;
    w->rows = h->H;
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
        return fail(code, "padded torus %d x %d (%zu bytes x2): %s", p.Wp, h->H, bytes, hipGetErrorString(e));
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
        w->paired_bands != h->paired_bands)
        for (int &c : w->auto_rpw) c = 0;
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
    h->last_variant = w->last_variant;
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
    if (mode == 1 && !pad_applies(h))
        return fail(GOLHIP_EINVAL, "the padded torus is for a whole torus without a communicator whose width is no "
                                   "multiple of 32 (width %d, rows %d of %d)", h->W, h->rows, h->H);
    h->pad_mode = mode;
    h->pad_nomem = false;
    return GOLHIP_OK;
}

}  // extern "C"
