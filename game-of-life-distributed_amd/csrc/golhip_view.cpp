// golhip_view.cpp — live view (K7, gol_view.hip): frames of one handle and of
// a board held as n row strips.
#include "golhip_impl.h"

namespace gh GOLHIP_HIDDEN {

// ---------------------------------------------------------------------------
// live view (K7, gol_view.hip)
// ---------------------------------------------------------------------------
// The rules of a frame on a W x H torus: format, scale, frame size, origin, one lap at most.
static int view_rules(const golhip_view_t *v, int W, int H) {
    if (!v) return fail(GOLHIP_EINVAL, "view is null");
    if (v->format != GOLHIP_VIEW_ARGB8888 && v->format != GOLHIP_VIEW_GRAY8)
        return fail(GOLHIP_EINVAL, "view format %d", v->format);
    if (v->scale < 1 || v->scale > GOLHIP_VIEW_MAX_SCALE)
        return fail(GOLHIP_EINVAL, "view scale %d not in [1, %d]", v->scale, GOLHIP_VIEW_MAX_SCALE);
    if (v->out_w < 1 || v->out_h < 1) return fail(GOLHIP_EINVAL, "view frame %d x %d", v->out_w, v->out_h);
    if (v->x0 < 0 || v->x0 >= W || v->y0 < 0 || v->y0 >= H)
        return fail(GOLHIP_EINVAL, "view origin (%d, %d) outside the %d x %d board", v->x0, v->y0, W, H);
    if ((int64_t)v->out_w * v->scale > W || (int64_t)v->out_h * v->scale > H)
        return fail(GOLHIP_EINVAL, "view of %d x %d pixels at scale %d is more than one lap of the %d x %d board",
                    v->out_w, v->out_h, v->scale, W, H);
    return GOLHIP_OK;
}

// Checks a view against the handle (h->mu held); *bytes = one frame.
static int view_check(golhip_t h, const golhip_view_t *v, uint64_t *bytes) {
    if (int rc = view_rules(v, h->W, h->H)) return rc;
    if (h->rows != h->H &&
        (v->y0 < h->row0 || (int64_t)v->y0 + (int64_t)v->out_h * v->scale > (int64_t)h->row0 + h->rows))
        return fail(GOLHIP_EINVAL, "view rows [%d, %lld) leave the strip's rows [%d, %d)", v->y0,
                    (long long)v->y0 + (long long)v->out_h * v->scale, h->row0, h->row0 + h->rows);
    if (!h->loaded) return fail(GOLHIP_EINVAL, "no board loaded");
    *bytes = (uint64_t)v->out_w * (uint64_t)v->out_h * (v->format == GOLHIP_VIEW_GRAY8 ? 1u : 4u);
    return GOLHIP_OK;
}

// The kernel arguments a handle and a view fix: all but the output and its rows (out, y0, out_h).
static golk::ViewArgs view_args(golhip_t h, const golhip_view_t *v) {
    golk::ViewArgs a{};
    a.rows = h->cur_rows();
    a.W = h->W;
    a.Ww = h->Ww;
    a.H = h->rows;
    a.x0 = v->x0;
    a.s = v->scale;
    a.out_w = v->out_w;
    a.il = h->il;
    a.format = v->format;
    return a;
}

// Enqueue one frame of the current board into device-visible memory `dst`.
static int view_launch(golhip_t h, const golhip_view_t *v, void *dst) {
    golk::ViewArgs a = view_args(h, v);
    a.out = dst;
    a.y0 = v->y0 - h->row0;
    a.out_h = v->out_h;
    if (int rc = span_begin(h, h->stream)) return rc;
    const hipError_t e = golk::launch_view(a, h->stream);
    if (e != hipSuccess) return fail(GOLHIP_EHIP, "view launch: %s", hipGetErrorString(e));
    if (int rc = span_end(h, 4, true)) return rc;
    h->n.view_frames++;
    return GOLHIP_OK;
}

// One frame to `out` (host): written there by the kernel if it is
// golhip_host_alloc memory (`mapped`: its device address), else staged.
static int view_to_host(golhip_t h, const golhip_view_t *v, void *out, void *mapped, uint64_t bytes) {
    if (mapped) return view_launch(h, v, mapped);
    if (int rc = h->d_stage.ensure(h, (int64_t)bytes)) return rc;
    if (int rc = view_launch(h, v, h->d_stage.p)) return rc;
    HIP_OR_FAIL(hipMemcpyAsync(out, h->d_stage.p, (size_t)bytes, hipMemcpyDeviceToHost, h->stream));
    return GOLHIP_OK;
}

// ---------------------------------------------------------------------------
// live view of a board held as n row strips (golhip_group_view_*)
// ---------------------------------------------------------------------------
// The viewport's rows, one lap at most, cut at the strip boundaries.  A run of
// whole pixel rows inside one strip is a Whole: the strip renders it straight
// into the frame.  What is left of a strip's run at either end is a Part: rows
// [r_lo, r_hi) of pixel row py, rendered as a count row (slot `slot` of the
// seam buffer).  The parts of one pixel row are consecutive and take
// consecutive slots; a SeamRow lists them.  A strip has at most two runs (the
// viewport ends in the strip it began in), so at most two Wholes, four Parts.
struct ViewWhole {
    int strip, py, npy, ylocal;  // ylocal: the strip's local row of pixel row py's row 0
};
struct ViewPart {
    int strip, py, r_lo, r_hi, ylocal, slot;
};
struct ViewSeamRow {
    int py, slot, k;
};
struct GroupViewPlan {
    std::vector<ViewWhole> wholes;
    std::vector<ViewPart> parts;
    std::vector<ViewSeamRow> seams;
    int first = 0;   // the strip that holds row y0: it resolves
    int cw = 0;      // words of a count row
    uint64_t bpp = 4, bytes = 0;
};

static void group_view_plan(golhip_t *hs, int n, const golhip_view_t *v, GroupViewPlan *p) {
    const int s = v->scale;
    int i = 0;
    while (!(v->y0 >= hs[i]->row0 && v->y0 < hs[i]->row0 + hs[i]->rows)) ++i;
    p->first = i;
    p->cw = golk::view_count_stride(v->out_w);
    p->bpp = v->format == GOLHIP_VIEW_GRAY8 ? 1 : 4;
    p->bytes = (uint64_t)v->out_w * (uint64_t)v->out_h * p->bpp;
    int64_t rel = 0, left = (int64_t)v->out_h * s;
    int cur = v->y0;
    while (left > 0) {
        const int64_t end = rel + std::min<int64_t>(left, hs[i]->row0 + hs[i]->rows - cur);  // this run: [rel, end)
        int64_t r = rel;
        auto local = [&](int64_t at) { return (int)(cur - hs[i]->row0 + (at - rel)); };  // local row of view row `at`
        if (r % s != 0) {  // the end of a pixel row begun in the strip before
            const int py = (int)(r / s);
            const int64_t hi = std::min<int64_t>(end, (int64_t)(py + 1) * s);
            p->parts.push_back({i, py, (int)(r - (int64_t)py * s), (int)(hi - (int64_t)py * s), local((int64_t)py * s), 0});
            r = hi;
        }
        if (const int npy = (int)((end - r) / s)) {
            p->wholes.push_back({i, (int)(r / s), npy, local(r)});
            r += (int64_t)npy * s;
        }
        if (r < end) {  // the start of a pixel row that the next strip goes on with
            p->parts.push_back({i, (int)(r / s), 0, (int)(end - r), local(r), 0});
        }
        left -= end - rel;
        cur += (int)(end - rel);
        rel = end;
        if (cur == hs[i]->row0 + hs[i]->rows) {  // on into the next strip, past the last into the first
            i = (i + 1) % n;
            cur = hs[i]->row0;
        }
    }
    for (size_t j = 0; j < p->parts.size(); ++j) {
        p->parts[j].slot = (int)j;
        if (p->seams.empty() || p->seams.back().py != p->parts[j].py)
            p->seams.push_back({p->parts[j].py, (int)j, 1});
        else
            p->seams.back().k++;
    }
}

// Checks of both group view calls, before any mutex is taken (as
// group_step_impl reads its strips); *torus: the group is one whole-torus
// handle and the call is the single-handle one.
static int group_view_check(golhip_t *hs, int32_t n, const golhip_view_t *v, bool *torus) {
    if (int rc = group_check(hs, n)) return rc;
    *torus = n == 1 && hs[0]->torus();
    if (*torus) return GOLHIP_OK;
    for (int i = 0; i < n; ++i) {
        if (hs[i]->turns != hs[0]->turns)
            return fail(GOLHIP_EINVAL, "strip %d is at turn %lld, strip 0 at turn %lld", i, (long long)hs[i]->turns,
                        (long long)hs[0]->turns);
        if (want_il(hs[i]) != want_il(hs[0])) return fail(GOLHIP_EINVAL, "strip %d uses another word layout", i);
    }
    return view_rules(v, hs[0]->W, hs[0]->H);
}

// Events of one group view call: part[i] after strip i's count rows have
// reached the seam buffer, `resolved` after the resolve kernel has read them.
struct GroupViewEvents {
    std::vector<hipEvent_t> part;
    hipEvent_t resolved = nullptr;
    bool resolved_set = false;
};

// Enqueue one frame of the strips' current boards to `out` (host; `mapped`:
// its device address in golhip_host_alloc memory mapped on `mapped_dev`, or
// null).  Every strip's mutex is held; nothing is synchronised.
static int group_view_enqueue(golhip_t *hs, int n, const golhip_view_t *v, const GroupViewPlan &p, GroupViewEvents &ev,
                              void *out, void *mapped, int mapped_dev) {
    golhip *res = hs[p.first];
    const int64_t row_bytes = (int64_t)v->out_w * (int64_t)p.bpp;
    const int64_t seam_words = (int64_t)p.parts.size() * p.cw;
    if (seam_words) {
        if (int rc = set_dev(res)) return rc;
        if (int rc = res->d_vcount.ensure(res, seam_words)) return rc;
    }
    for (int i = 0; i < n; ++i) {
        golhip *h = hs[i];
        bool any = false, any_part = false;
        for (const ViewWhole &w : p.wholes) any |= w.strip == i;
        for (const ViewPart &q : p.parts) any_part |= q.strip == i;
        if (!any && !any_part) continue;
        if (int rc = set_dev(h)) return rc;
        const bool direct = mapped && h->device == mapped_dev;
        // staging: this strip's whole pixel rows, then (the resolving strip) the seam rows
        int64_t stage_bytes = 0;
        std::vector<int64_t> whole_off;
        for (const ViewWhole &w : p.wholes)
            if (w.strip == i) {
                whole_off.push_back(stage_bytes);
                stage_bytes += ((int64_t)w.npy * row_bytes + 15) / 16 * 16;
            }
        if (i == p.first) stage_bytes += (int64_t)p.seams.size() * row_bytes;
        if (!direct)
            if (int rc = h->d_stage.ensure(h, std::max<int64_t>(stage_bytes, 16))) return rc;
        const bool peer = any_part && h->device != res->device;  // count rows travel to the resolving strip's device
        if (peer)
            if (int rc = h->d_vcount.ensure(h, seam_words)) return rc;
        // the seam buffer is reused from frame to frame: no count row of this
        // frame before the last frame's resolve has read the buffer
        if (any_part && i != p.first && ev.resolved_set) HIP_OR_FAIL(hipStreamWaitEvent(h->stream, ev.resolved, 0));
        if (int rc = span_begin(h, h->stream)) return rc;
        for (const ViewPart &q : p.parts) {
            if (q.strip != i) continue;
            golk::ViewArgs a = view_args(h, v);
            uint32_t *dst = (peer ? h->d_vcount.p : res->d_vcount.p) + (int64_t)q.slot * p.cw;
            a.out = dst;
            a.y0 = q.ylocal;
            a.out_h = 1;
            a.r_lo = q.r_lo;
            a.r_hi = q.r_hi;
            const hipError_t e = golk::launch_view_counts(a, h->stream);
            if (e != hipSuccess) return fail(GOLHIP_EHIP, "view counts launch (strip %d): %s", i, hipGetErrorString(e));
            if (peer)
                HIP_OR_FAIL(hipMemcpyPeerAsync(res->d_vcount.p + (int64_t)q.slot * p.cw, res->device, dst, h->device,
                                               (size_t)p.cw * sizeof(uint32_t), h->stream));
        }
        size_t wi = 0;
        for (const ViewWhole &w : p.wholes) {
            if (w.strip != i) continue;
            golk::ViewArgs a = view_args(h, v);
            a.out = direct ? (void *)((char *)mapped + (int64_t)w.py * row_bytes) : (void *)(h->d_stage.p + whole_off[wi]);
            a.y0 = w.ylocal;
            a.out_h = w.npy;
            const hipError_t e = golk::launch_view(a, h->stream);
            if (e != hipSuccess) return fail(GOLHIP_EHIP, "view launch (strip %d): %s", i, hipGetErrorString(e));
            ++wi;
        }
        if (int rc = span_end(h, 4, true)) return rc;
        h->n.view_frames++;
        if (any_part && i != p.first) HIP_OR_FAIL(hipEventRecord(ev.part[i], h->stream));
        if (!direct) {
            wi = 0;
            for (const ViewWhole &w : p.wholes) {
                if (w.strip != i) continue;
                HIP_OR_FAIL(hipMemcpyAsync((char *)out + (int64_t)w.py * row_bytes, h->d_stage.p + whole_off[wi],
                                           (size_t)((int64_t)w.npy * row_bytes), hipMemcpyDeviceToHost, h->stream));
                ++wi;
            }
        }
    }
    if (p.seams.empty()) return GOLHIP_OK;
    // resolve on the first strip's stream, behind every other strip's count rows
    golhip *h = res;
    if (int rc = set_dev(h)) return rc;
    std::vector<bool> waited(n, false);
    for (const ViewPart &q : p.parts)
        if (q.strip != p.first && !waited[q.strip]) {
            HIP_OR_FAIL(hipStreamWaitEvent(h->stream, ev.part[q.strip], 0));
            waited[q.strip] = true;
        }
    const bool direct = mapped && h->device == mapped_dev;
    int64_t seam_off = 0;
    for (const ViewWhole &w : p.wholes)
        if (w.strip == p.first) seam_off += ((int64_t)w.npy * row_bytes + 15) / 16 * 16;
    if (int rc = span_begin(h, h->stream)) return rc;
    for (size_t j0 = 0; j0 < p.seams.size(); j0 += golk::kViewResolveRows) {
        golk::ViewResolveArgs r{};
        r.counts = h->d_vcount.p;
        r.cw = p.cw;
        r.out_w = v->out_w;
        r.s = v->scale;
        r.format = v->format;
        r.nrows = (int)std::min<size_t>(golk::kViewResolveRows, p.seams.size() - j0);
        // staged: seam row j is row j of a frame of seam rows only
        r.out = direct ? mapped : (void *)(h->d_stage.p + seam_off);
        for (int j = 0; j < r.nrows; ++j) {
            r.py[j] = direct ? p.seams[j0 + j].py : (int)(j0 + j);
            r.slot[j] = p.seams[j0 + j].slot;
            r.k[j] = p.seams[j0 + j].k;
        }
        const hipError_t e = golk::launch_view_resolve(r, h->stream);
        if (e != hipSuccess) return fail(GOLHIP_EHIP, "view resolve launch: %s", hipGetErrorString(e));
    }
    if (int rc = span_end(h, 4, true)) return rc;
    HIP_OR_FAIL(hipEventRecord(ev.resolved, h->stream));
    ev.resolved_set = true;
    if (!direct)
        for (size_t j = 0; j < p.seams.size(); ++j)
            HIP_OR_FAIL(hipMemcpyAsync((char *)out + (int64_t)p.seams[j].py * row_bytes,
                                       h->d_stage.p + seam_off + (int64_t)j * row_bytes, (size_t)row_bytes,
                                       hipMemcpyDeviceToHost, h->stream));
    return GOLHIP_OK;
}

static int group_view_events(golhip_t *hs, int n, int first, GroupViewEvents *ev) {
    ev->part.assign(n, nullptr);
    for (int i = 0; i < n; ++i) {
        HIP_OR_FAIL(hipSetDevice(hs[i]->device));
        HIP_OR_FAIL(hipEventCreateWithFlags(&ev->part[i], hipEventDisableTiming));
    }
    HIP_OR_FAIL(hipSetDevice(hs[first]->device));
    HIP_OR_FAIL(hipEventCreateWithFlags(&ev->resolved, hipEventDisableTiming));
    return GOLHIP_OK;
}

// Synchronises every strip's stream, reports its flags, destroys the events.
static int group_view_finish(golhip_t *hs, int n, GroupViewEvents *ev, int rc) {
    for (int i = 0; i < n; ++i) {
        HIP_RC(hipSetDevice(hs[i]->device));
        HIP_RC(hipStreamSynchronize(hs[i]->stream));
        if (!rc) rc = take_skew_err(hs[i]);
    }
    for (hipEvent_t e : ev->part)
        if (e) HIP_RC(hipEventDestroy(e));
    if (ev->resolved) HIP_RC(hipEventDestroy(ev->resolved));
    return rc;
}

}  // namespace gh

using namespace gh;

extern "C" {

int golhip_view_frame(golhip_t h, const golhip_view_t *v, void *out, uint64_t cap_bytes, int64_t *at_turn) {
    if (int rc = check(h)) return rc;
    if (!out) return fail(GOLHIP_EINVAL, "out is null");
    std::lock_guard<std::mutex> g(h->mu);
    uint64_t bytes = 0;
    if (int rc = view_check(h, v, &bytes)) return rc;
    if (cap_bytes < bytes)
        return fail(GOLHIP_ERANGE, "buffer holds %llu bytes, the frame needs %llu", (unsigned long long)cap_bytes,
                    (unsigned long long)bytes);
    if (int rc = set_dev(h)) return rc;
    if (int rc = view_to_host(h, v, out, mapped_device_ptr(out, (size_t)bytes), bytes)) return rc;
    if (int rc = sync_stream(h)) return rc;
    if (at_turn) *at_turn = h->turns;
    return GOLHIP_OK;
}

int golhip_view_stream(golhip_t h, int64_t nturns, int64_t every, const golhip_view_t *v, void *out,
                       uint64_t cap_frames, uint64_t *frames, int64_t *turns_done) {
    if (int rc = check(h)) return rc;
    if (frames) *frames = 0;
    if (turns_done) *turns_done = 0;
    if (nturns < 0) return fail(GOLHIP_EINVAL, "nturns %lld", (long long)nturns);
    if (every < 1) return fail(GOLHIP_EINVAL, "every %lld", (long long)every);
    std::lock_guard<std::mutex> g(h->mu);
    uint64_t bytes = 0;
    if (int rc = view_check(h, v, &bytes)) return rc;
    if (h->nranks == 1 && !h->torus()) return fail(GOLHIP_EINVAL, "strip handle needs golhip_comm_init or golhip_group_step");
    const uint64_t nf = (uint64_t)(nturns / every);
    if (nf > cap_frames)
        return fail(GOLHIP_ERANGE, "buffer holds %llu frames, %lld turns at every %lld need %llu",
                    (unsigned long long)cap_frames, (long long)nturns, (long long)every, (unsigned long long)nf);
    if (nf > 0 && !out) return fail(GOLHIP_EINVAL, "out is null");
    if (int rc = set_dev(h)) return rc;
    char *mapped = nf ? (char *)mapped_device_ptr(out, (size_t)(nf * bytes)) : nullptr;
    const int64_t turns0 = h->turns;
    for (uint64_t f = 0; f < nf; ++f) {
        if (int rc = step_checked_locked(h, every, 0)) return rc;
        if (int rc = view_to_host(h, v, (char *)out + f * bytes, mapped ? mapped + f * bytes : nullptr, bytes)) return rc;
    }
    if (int rc = step_checked_locked(h, nturns - (int64_t)nf * every, 0)) return rc;
    if (nf > 0)
        if (int rc = sync_stream(h)) return rc;
    if (frames) *frames = nf;
    if (turns_done) *turns_done = h->turns - turns0;
    return GOLHIP_OK;
}

int golhip_group_view_frame(golhip_t *hs, int32_t n, const golhip_view_t *v, void *out, uint64_t cap_bytes,
                            int64_t *at_turn) {
    bool torus = false;
    if (int rc = group_view_check(hs, n, v, &torus)) return rc;
    if (torus) return golhip_view_frame(hs[0], v, out, cap_bytes, at_turn);
    if (!out) return fail(GOLHIP_EINVAL, "out is null");
    GroupViewPlan p;
    group_view_plan(hs, n, v, &p);
    if (cap_bytes < p.bytes)
        return fail(GOLHIP_ERANGE, "buffer holds %llu bytes, the frame needs %llu", (unsigned long long)cap_bytes,
                    (unsigned long long)p.bytes);
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    int mapped_dev = -1;
    void *mapped = mapped_device_ptr(out, (size_t)p.bytes, &mapped_dev);
    GroupViewEvents ev;
    int rc = group_view_events(hs, n, p.first, &ev);
    if (!rc) rc = group_view_enqueue(hs, n, v, p, ev, out, mapped, mapped_dev);
    rc = group_view_finish(hs, n, &ev, rc);
    if (!rc && at_turn) *at_turn = hs[0]->turns;
    return rc;
}

int golhip_group_view_stream(golhip_t *hs, int32_t n, int64_t nturns, int64_t every, const golhip_view_t *v, void *out,
                             uint64_t cap_frames, uint64_t *frames, int64_t *turns_done) {
    if (frames) *frames = 0;
    if (turns_done) *turns_done = 0;
    bool torus = false;
    if (int rc = group_view_check(hs, n, v, &torus)) return rc;
    if (torus) return golhip_view_stream(hs[0], nturns, every, v, out, cap_frames, frames, turns_done);
    if (nturns < 0) return fail(GOLHIP_EINVAL, "nturns %lld", (long long)nturns);
    if (every < 1) return fail(GOLHIP_EINVAL, "every %lld", (long long)every);
    GroupViewPlan p;
    group_view_plan(hs, n, v, &p);
    const uint64_t nf = (uint64_t)(nturns / every);
    if (nf > cap_frames)
        return fail(GOLHIP_ERANGE, "buffer holds %llu frames, %lld turns at every %lld need %llu",
                    (unsigned long long)cap_frames, (long long)nturns, (long long)every, (unsigned long long)nf);
    if (nf > 0 && !out) return fail(GOLHIP_EINVAL, "out is null");
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    int mapped_dev = -1;
    char *mapped = nf ? (char *)mapped_device_ptr(out, (size_t)(nf * p.bytes), &mapped_dev) : nullptr;
    const int64_t turns0 = hs[0]->turns;
    GroupViewEvents ev;
    std::vector<hipEvent_t> ready(n, nullptr);  // group_step_locked's, kept over the whole run
    int rc = group_view_events(hs, n, p.first, &ev);
    for (int i = 0; i < n; ++i) {
        HIP_RC(hipSetDevice(hs[i]->device));
        HIP_RC(hipEventCreateWithFlags(&ready[i], hipEventDisableTiming));
    }
    for (uint64_t f = 0; f < nf && !rc; ++f) {
        rc = group_step_locked(hs, n, every, 0, ready.data());
        if (!rc)
            rc = group_view_enqueue(hs, n, v, p, ev, (char *)out + f * p.bytes, mapped ? mapped + f * p.bytes : nullptr,
                                    mapped_dev);
    }
    if (!rc) rc = group_step_locked(hs, n, nturns - (int64_t)nf * every, 0, ready.data());
    rc = group_view_finish(hs, n, &ev, rc);
    for (hipEvent_t e : ready)
        if (e) HIP_RC(hipEventDestroy(e));
    if (rc) return rc;
    if (frames) *frames = nf;
    if (turns_done) *turns_done = hs[0]->turns - turns0;
    return GOLHIP_OK;
}

}  // extern "C"
