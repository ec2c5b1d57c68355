// golhip_step.cpp — the turn loop: per-launch, resident (K1p) and LDS-band
// (K1r) step launches, the resident-launch guard, the RCCL ring and the
// in-process group step.
#include "golhip_impl.h"

namespace gh GOLHIP_HIDDEN {

// torus mode: the handle holds the whole board and wraps rows itself;
// halo mode: rows outside the strip come from the halo rows.
golk::StepArgs step_args(golhip_t h, unsigned long long *alive, bool halo) {
    golk::StepArgs a{};
    a.src = h->buf[h->cur];
    a.dst = h->buf[h->cur ^ 1];
    a.W = h->W;
    a.Ww = h->Ww;
    a.rows_out = h->rows;
    a.dst_base = kHalo;
    if (!halo) {
        a.in.base = kHalo;
        a.in.wrap = h->H;
        a.in.off = 0;
        a.in.rmax = h->H - 1;
    } else {
        a.in.base = 0;
        a.in.wrap = 0;
        a.in.off = kHalo;
        a.in.rmax = (int)h->phys_rows - 1;
    }
    a.rows_per_wave = h->rows_per_wave;
    a.dummy_rows = h->dummy_rows > 0 ? h->dummy_rows : kHalo;
    a.alive = alive;
    a.count_lo = 0;
    a.count_hi = a.rows_out;
    return a;
}

// RCCL halo exchange for a launch of `depth` turns on stream `st`.  Posting
// order pairs correctly even when prev == next (2 ranks) or both are this
// rank (one-rank ring, option "force_halo"): on every A->B channel the first
// message is A's top rows (B's bottom halo), the second A's bottom rows.
int exchange_rccl(golhip_t h, int depth, hipStream_t st) {
    if (h->halo_skip) return GOLHIP_OK;  // measurement only (option "halo_skip")
    golhip_halo_plan_t p;
    halo_plan(h->rows, h->nranks, h->rank, depth, h->Ww, &p);
    uint32_t *b = h->buf[h->cur];
    const size_t n = (size_t)depth * h->Ww;
    if (int rc = span_begin(h, st)) return rc;
    if (h->xport) {
        // test transport: the two send blocks to pinned memory, the callback
        // trades them for the neighbours', the two receive blocks back
        if ((int64_t)n > h->xport_cap) {
            HIP_OR_FAIL(hipHostFree(h->xport_host));
            h->xport_host = nullptr;
            h->xport_cap = 0;
            HIP_OR_FAIL(hipHostMalloc(&h->xport_host, 4 * n * 4, hipHostMallocDefault));
            h->xport_cap = (int64_t)n;
        }
        uint32_t *hb = h->xport_host;
        const size_t bytes = n * 4;
        HIP_OR_FAIL(hipMemcpyAsync(hb, b + (int64_t)p.send_up_row * h->Ww, bytes, hipMemcpyDeviceToHost, st));
        HIP_OR_FAIL(hipMemcpyAsync(hb + n, b + (int64_t)p.send_down_row * h->Ww, bytes, hipMemcpyDeviceToHost, st));
        HIP_OR_FAIL(hipStreamSynchronize(st));
        if (int r = h->xport(h->xport_user, p.prev_rank, p.next_rank, hb, hb + n, hb + 2 * n, hb + 3 * n,
                             (int64_t)bytes))
            return fail(GOLHIP_ERCCL, "test transport returned %d", r);
        HIP_OR_FAIL(hipMemcpyAsync(b + (int64_t)p.recv_top_row * h->Ww, hb + 2 * n, bytes, hipMemcpyHostToDevice, st));
        HIP_OR_FAIL(hipMemcpyAsync(b + (int64_t)p.recv_bottom_row * h->Ww, hb + 3 * n, bytes, hipMemcpyHostToDevice, st));
        HIP_OR_FAIL(hipStreamSynchronize(st));  // the pinned blocks are reused by the next exchange
    } else {
        NCCL_OR_FAIL(ncclGroupStart());
        NCCL_OR_FAIL(ncclSend(b + (int64_t)p.send_up_row * h->Ww, n, ncclUint32, p.prev_rank, h->comm, st));
        NCCL_OR_FAIL(ncclRecv(b + (int64_t)p.recv_bottom_row * h->Ww, n, ncclUint32, p.next_rank, h->comm, st));
        NCCL_OR_FAIL(ncclSend(b + (int64_t)p.send_down_row * h->Ww, n, ncclUint32, p.next_rank, h->comm, st));
        NCCL_OR_FAIL(ncclRecv(b + (int64_t)p.recv_top_row * h->Ww, n, ncclUint32, p.prev_rank, h->comm, st));
        NCCL_OR_FAIL(ncclGroupEnd());
    }
    if (int rc = span_end(h, 3)) return rc;
    h->n.halo_bytes += 2 * (int64_t)n * 4;
    h->n.halo_exchanges++;
    return GOLHIP_OK;
}

// Halo mode: output rows [lo, hi) instead of [0, rows) (the deep-halo
// extension), counting only [0, rows).
static void shift_rows(golk::StepArgs &a, int lo, int hi) {
    const int rows = a.rows_out;  // the handle's rows (step_args)
    a.rows_out = hi - lo;
    a.dst_base = kHalo + lo;
    a.in.off = kHalo + lo;
    a.dummy_rows = std::max(1, std::min(a.dummy_rows, kHalo + std::min(lo, 0)));  // rows above the outputs
    a.count_lo = -lo;
    a.count_hi = -lo + rows;
}

// Launch the step kernel for output rows [lo, hi) of this handle (halos, if
// used, already in place); `alive` (nullable) accumulates their popcount.
// No bookkeeping: see finish_launch.
static int launch_rows(golhip_t h, int depth, unsigned long long *alive, bool halo, int lo, int hi) {
    const hipStream_t st = h->stream;
    golk::StepArgs a = step_args(h, alive, halo);
    if (lo != 0 || hi != h->rows) shift_rows(a, lo, hi);
    const int wpl = wpl_for(h);
    const bool rule = h->rule_path();  // K11: canonical words, one word per lane, plain bands
    const bool dyn = h->rule_kernel == 2;
    if (a.rows_out == h->rows) {
        a.rows_per_wave = rows_per_wave_for(h, depth);
    } else if (h->rows_per_wave > 0) {
        a.rows_per_wave = h->rows_per_wave;
    } else if (rule) {
        const int slots = h->cu_count * (h->plane ? golk::plane_wave_slots_per_cu(depth, h->birth, h->survive, dyn)
                                                  : golk::rule_wave_slots_per_cu(depth, h->W, h->birth, h->survive, dyn));
        a.rows_per_wave = golk::auto_rows_per_wave(h->Ww, a.rows_out, depth, std::max(slots, 1), false, 1, false);
    } else {
        const int slots = h->cu_count * golk::tb_wave_slots_per_cu(depth, wpl, tb_paired(h));
        a.rows_per_wave = golk::auto_rows_per_wave(h->Ww, a.rows_out, depth, std::max(slots, 1), h->fill_skip, wpl,
                                                     tb_paired(h));
    }
    // a wave's buffer-store range (two bands of a paired region) must stay < 2 GiB
    a.rows_per_wave = (int)std::min<int64_t>(a.rows_per_wave, ((1ll << 31) - 1) / (8ll * h->Ww));
    if (rule && h->il != 0) return fail(GOLHIP_EINVAL, "the rule kernel steps canonical words (layout %d)", h->il);
    if (int rc = span_begin(h, st)) return rc;
    hipError_t e;
    golk::SkewArgs sk{};
    const bool skew = !rule && skew_plan(h, depth, wpl, a, &sk);
    if (rule && h->plane) {
        // K15: the board row of the frame's row 0 (negative in a deep-halo launch of the first strip) and H
        e = golk::launch_step_plane(a, depth, h->birth, h->survive, h->row0 + lo, h->H, st, dyn);
    } else if (rule) {
        e = golk::launch_step_rule(a, depth, h->birth, h->survive, st, dyn);
    } else if (skew) {
        sk.base = a;
        e = golk::launch_skew(sk, depth, wpl, st);
    } else if (h->W % 32 == 0) {
        e = golk::launch_step_tb(a, depth, st, h->fill_skip, wpl, tb_paired(h));
    } else {
        e = golk::launch_step_generic(a, st);
    }
    h->last_variant = rule ? (h->plane ? 6 : 5) : h->W % 32 != 0 ? 0 : skew ? 3 : 1;
    if (e != hipSuccess) return fail(GOLHIP_EHIP, "step launch: %s", hipGetErrorString(e));
    if (int rc = span_end(h, 0, true)) return rc;
    h->n.step_launches++;
    h->n.rule_launches += rule;
    h->n.skew_launches += skew;
    h->n.skew_half_launches += skew && sk.half;
    if (skew && sk.pairs) {
        h->n.pair_launches++;
        h->n.pair_turns += depth;
    }
    return GOLHIP_OK;
}

static void finish_launch(golhip_t h, int depth, bool count) {
    h->cur ^= 1;
    h->turns += depth;
    h->n.step_turns += depth;
    if (count) h->alive_turn = h->turns;
}

// One step launch of `depth` turns (halos already in place).
int launch_depth(golhip_t h, int depth, bool count, bool halo) {
    unsigned long long *alive = nullptr;
    if (count) {
        alive = h->d_scalars;
        HIP_OR_FAIL(hipMemsetAsync(alive, 0, sizeof(unsigned long long), h->stream));
    }
    if (int rc = launch_rows(h, depth, alive, halo, 0, h->rows)) return rc;
    finish_launch(h, depth, count);
    return GOLHIP_OK;
}

static int launch_ext(golhip_t h, int depth, bool count, int ext) {
    unsigned long long *alive = nullptr;
    if (count) {
        alive = h->d_scalars;
        HIP_OR_FAIL(hipMemsetAsync(alive, 0, sizeof(unsigned long long), h->stream));
    }
    if (int rc = launch_rows(h, depth, alive, true, -ext, h->rows + ext)) return rc;
    finish_launch(h, depth, count);
    return GOLHIP_OK;
}

// The words the resident kernels (K1p, K1r) synchronise through: d_sync
// ([0] error, then one progress word per workgroup / band: 2 dev_cu + 2 in
// all) and the pinned copy of the error word.  False if they cannot be had.
static bool ensure_sync_words(golhip_t h) {
    if (h->d_sync) return true;
    if (hipMalloc(&h->d_sync, (size_t)(2 * h->dev_cu + 2) * sizeof(unsigned)) != hipSuccess ||
        hipHostMalloc(&h->h_err, sizeof(unsigned), hipHostMallocDefault) != hipSuccess)
        return false;
    *h->h_err = 0;
    return true;
}

// Test hook "resident_fault": 1 = every resident launch's band / workgroup 0
// never reports, 2 = only the first launch of a guarded step (a transient
// starvation: the step's later launches are healthy and must not hide it).
static int resident_fault_now(golhip_t h, bool first) {
    return h->resident_fault == 1 || (h->resident_fault == 2 && first) ? 1 : 0;
}

// One resident launch of J super-steps of `depth` turns over the rows of
// `base` (count: the popcount of its last super-step goes to d_scalars);
// returns false (with *rc == 0) when no workgroup plan fits.
static bool persist_launch(golhip_t h, golk::StepArgs base, int64_t J, int depth, int wpl, bool count, int *rc,
                           bool half_last = false) {
    *rc = GOLHIP_OK;
    const int nw = persist_nw_for(h, depth, wpl);
    if (golk::persist_blocks_per_cu(depth, wpl, nw) < 1) return false;
    golk::PersistArgs p{};
    // Unpaired fallback: with two waves per SIMD the older one is served
    // first, so the older half of the waves gets 65 % of the rows.
    const int age_split = nw == 8 ? 65 : 0;
    const bool split = age_split > 0 && age_split < 100;
    if (!golk::plan_persist(h->Ww, base.rows_out, depth, h->cu_count, wpl, nw, &p, h->persist_wg_tx)) return false;
    if (2ll * p.S * h->Ww * 4 >= (1ll << 31)) return false;  // a band's buffer-store range
    // every workgroup must be resident at once (they wait on their neighbours):
    // the grid may not exceed what the occupancy query admits on this device
    if ((int64_t)p.cols * p.wg_y > (int64_t)golk::persist_blocks_per_cu(depth, wpl, nw) * h->cu_count) return false;
    if (h->paired_bands && p.wg_sy >= 2 && p.wg_sy % 2 == 0) {
        // the older and the younger wave of a SIMD stream a shared two-band
        // region from both ends and meet where the arbiter's service put them
        p.paired = 1;
    } else if (split && p.wg_sy >= 2 && p.wg_sy % 2 == 0) {
        // rows of a workgroup stack: age_split % to the band rows of the
        // NW/2 oldest waves (w < NW/2 <=> band row < wg_sy/2)
        const int R = p.wg_sy * p.S, hr = p.wg_sy / 2;
        p.S_old = std::max(1, (int)((int64_t)R * age_split / 100 / hr));
        p.S_young = std::max(1, (R - hr * p.S_old) / (p.wg_sy - hr));
        if (hr * p.S_old >= R) p.S_old = p.S_young = 0;
    }
    p.nw = nw;
    if (!ensure_sync_words(h)) {
        *rc = fail(GOLHIP_ENOMEM, "persistent sync words");
        return false;
    }
    if (count) {
        hipError_t e = hipMemsetAsync(h->d_scalars, 0, sizeof(unsigned long long), h->stream);
        if (e != hipSuccess) { *rc = fail(GOLHIP_EHIP, "memset: %s", hipGetErrorString(e)); return false; }
    }
    const int e0w = h->err_clear ? 0 : 1;  // the error word is sticky over the guarded step
    h->err_clear = false;
    hipError_t e = hipMemsetAsync(h->d_sync + e0w, 0, (size_t)(h->cu_count + 2 - e0w) * sizeof(unsigned), h->stream);
    const int fault = resident_fault_now(h, e0w == 0);
    p.base = base;
    p.base.alive = count ? h->d_scalars : nullptr;
    p.buf0 = h->buf[0];
    p.buf1 = h->buf[1];
    p.first = h->cur;
    p.J = (int)J;
    p.half_last = half_last ? 1 : 0;
    p.error = h->d_sync;
    p.progress = h->d_sync + 1;
    p.timeout_ticks = h->persist_timeout_ticks;
    p.trace = h->d_trace;
    p.fault = fault;
    if (e == hipSuccess && (*rc = span_begin(h, h->stream))) return false;
    if (e == hipSuccess) e = golk::launch_persist(p, depth, wpl, h->stream);
    if (e == hipSuccess && (*rc = span_end(h, 1))) return false;
    if (e == hipSuccess) e = hipMemcpyAsync(h->h_err, h->d_sync, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream);
    if (e != hipSuccess) {
        *rc = fail(GOLHIP_EHIP, "persistent launch: %s", hipGetErrorString(e));
        return false;
    }
    h->persist_pending = true;
    if (J & 1) h->cur ^= 1;
    const int64_t turns = J * depth - (half_last ? depth / 2 : 0);
    h->turns += turns;
    h->n.persist_turns += turns;
    h->n.persist_launches++;
    if (count) h->alive_turn = h->turns;
    return true;
}

// Keep the board recoverable before a step's first resident launch: a copy
// of this handle's rows that golhip_step restores (and then re-runs the step
// on the per-launch kernels) if a resident launch times out.  False (rc 0)
// if there is no room for the copy: then no resident launch this step.
// keeps_src: the step is one launch that never writes its source buffer (K1r,
// reads it once into LDS and writes only the other buffer) and nothing runs
// after it, so the source itself is the copy (a timeout leaves it intact).
static bool take_guard(golhip_t h, int *rc, bool keeps_src = false) {
    *rc = GOLHIP_OK;
    if (h->guarded) return true;  // a step of several resident launches keeps its first copy
    h->err_clear = true;          // the step's first resident launch clears the error word
    if (keeps_src) {
        h->guarded = true;
        h->guard_light = true;
        return true;
    }
    const size_t bytes = (size_t)h->local_words() * 4;
    if (h->backup.ensure(h, h->local_words())) return false;
    hipError_t e = hipMemcpyAsync(h->backup.p, h->cur_rows(), bytes, hipMemcpyDeviceToDevice, h->stream);
    if (e != hipSuccess) {
        *rc = fail(GOLHIP_EHIP, "resident-launch guard copy: %s", hipGetErrorString(e));
        return false;
    }
    h->guarded = true;
    return true;
}

// Torus: all `left` turns as one K1r launch (under the step guard, like
// K1p); returns the turns run (0 if K1r does not apply).
static int64_t try_lds(golhip_t h, int64_t left, bool count_last, int *rc) {
    *rc = GOLHIP_OK;
    if (left < 2 || !(h->il == 0 || h->il == 2)) return 0;
    const int64_t run = golk::resident_turns(left, h->resident_max);  // 32-bit super-step arithmetic in the kernel
    const int wpl = h->il == 2 ? 2 : 1;
    golk::LdsBandArgs p{};
    if (!lds_fits(h, wpl, &p)) return 0;
    const int64_t ew = golk::lds_band_edge_words(p.nb, p.D, p.stride);
    if (ew > h->lds_edge.cap) {
        if (h->lds_edge.release() != hipSuccess) {
            *rc = fail(GOLHIP_EHIP, "hipFree (K1r edges)");
            return 0;
        }
        if (h->lds_edge.ensure(h, ew)) return 0;  // no room for the edge rows: K1r does not apply
    }
    if (!ensure_sync_words(h)) {
        *rc = fail(GOLHIP_ENOMEM, "resident sync words");
        return 0;
    }
    if (!take_guard(h, rc, count_last && run == left)) return 0;
    const bool count = count_last && run == left;
    hipError_t e = count ? hipMemsetAsync(h->d_scalars, 0, sizeof(unsigned long long), h->stream) : hipSuccess;
    const int e0w = h->err_clear ? 0 : 1;  // the error word is sticky over the guarded step
    h->err_clear = false;
    if (e == hipSuccess) e = hipMemsetAsync(h->d_sync + e0w, 0, (size_t)(p.nb + 1 - e0w) * sizeof(unsigned), h->stream);
    p.fault = resident_fault_now(h, e0w == 0);
    p.src = h->cur_rows();
    p.dst = h->prev_rows();
    p.edge = h->lds_edge.p;
    p.error = h->d_sync;
    p.progress = h->d_sync + 1;
    p.alive = count ? h->d_scalars : nullptr;
    p.timeout_ticks = h->persist_timeout_ticks;
    p.turns = (int)run;
    p.trace = h->d_trace;
    if (e == hipSuccess && (*rc = span_begin(h, h->stream))) return 0;
    if (e == hipSuccess) e = golk::launch_lds_band(p, wpl, h->stream);
    if (e == hipSuccess && (*rc = span_end(h, 1))) return 0;
    if (e == hipSuccess) e = hipMemcpyAsync(h->h_err, h->d_sync, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream);
    if (e != hipSuccess) {
        *rc = fail(GOLHIP_EHIP, "resident LDS-band launch: %s", hipGetErrorString(e));
        return 0;
    }
    h->persist_pending = true;
    h->cur ^= 1;
    h->last_variant = 4;
    h->turns += run;
    h->n.persist_turns += run;
    h->n.persist_launches++;
    h->n.lds_launches++;
    if (count) h->alive_turn = h->turns;
    return run;
}

// Torus: J super-steps of `depth` turns in one resident launch; returns the
// turns run (0 if the persistent path does not apply).
static int64_t try_persist(golhip_t h, int64_t left, bool count_last, int *rc) {
    *rc = GOLHIP_OK;
    if (!persist_on(h) || h->W % 32 != 0 || !h->torus()) return 0;
    if (int64_t n = try_lds(h, left, count_last, rc)) return n;
    if (*rc) return 0;
    const int wpl = wpl_for(h);
    const int depth = persist_depth_for(h, wpl);
    if (depth < 4 || golk::persist_blocks_per_cu(depth, wpl, persist_nw_for(h, depth, wpl)) < 1) return 0;
    int64_t J = golk::resident_turns(left, h->resident_max) / depth;  // (32-bit super-step counts in the kernel)
    if (J < 2) return 0;
    // a remainder of exactly depth / 2 turns (1000 = 62 x 16 + 8) becomes a
    // last, half-depth super-step
    const bool half = h->persist_half && left - J * depth == depth / 2;
    if (half) ++J;
    const int64_t turns = J * depth - (half ? depth / 2 : 0);
    const bool count = count_last && turns == left;
    if (!take_guard(h, rc)) return 0;
    if (!persist_launch(h, step_args(h, nullptr, false), J, depth, wpl, count, rc, half)) {
        h->guarded = false;  // nothing resident ran: no check needed
        return 0;
    }
    return turns;
}

// Row strip between two deep-halo exchanges of k * d rows: the k launches of
// d turns as one resident launch of k super-steps over the rows
// [-(k-1) d, rows + (k-1) d) (the outer rows go stale one super-step at a
// time, as in the per-launch trapezoid, and are never read by a kept row).
// Only in the one-rank ring (force_halo), under the guard step_locked took
// at the start of the step: a timeout restores the board and re-runs the
// step on per-launch kernels, exchanges included, which is safe with no
// other rank.  Never in a multi-rank ring: a re-run on one rank alone would
// desynchronise the ring, so ring strips stay on per-launch kernels (K1w).
static bool try_persist_halo(golhip_t h, int d, int k, bool count, int *rc) {
    *rc = GOLHIP_OK;
    if (!persist_on(h) || h->W % 32 != 0 || k < 2 || d < 4) return false;
    if ((h->ringed() && h->nranks > 1) || !h->guarded) return false;
    const int wpl = wpl_for(h);
    if (d != persist_depth_for(h, wpl)) return false;
    const int e = (k - 1) * d;
    golk::StepArgs a = step_args(h, nullptr, true);
    shift_rows(a, -e, h->rows + e);
    return persist_launch(h, a, k, d, wpl, count, rc);
}

// golhip_step with h->mu held.
static int step_locked(golhip_t h, int64_t nturns, int32_t want_flips) {
    if (int rc = set_layout(h, want_il(h))) return rc;
    h->flips_valid = false;
    int64_t left = nturns;
    const int64_t tail = want_flips ? 1 : 0;
    const bool halo = h->halo_mode();
    if (pad_wanted(h, left - tail)) {
        // a width that is no multiple of 32 on the fast kernels (golhip_pad.cpp);
        // the last turn of a want_flips step runs on K1g below, as ever
        bool ran = false;
        if (int rc = pad_step(h, left - tail, &ran)) return rc;
        if (ran) left = tail;
    }
    if (!halo) {
        // resident launches while they apply (more than one only past
        // golk::kResidentMaxTurns turns), then per-launch kernels for the rest
        for (;;) {
            int rc = GOLHIP_OK;
            const int64_t n = try_persist(h, left - tail, tail == 0, &rc);
            if (rc) return rc;
            if (n <= 0) break;
            left -= n;
        }
    } else if (h->nranks == 1 && persist_on(h) && h->W % 32 == 0 && !h->guarded) {
        int rc = GOLHIP_OK;  // one-rank ring that may run resident launches: guard the step
        take_guard(h, &rc);
        if (rc) return rc;
    }
    // a whole torus on the pair rule's full tiles plans its tail from the pair
    // depths, and only then do 12 / 15 / 16 turns run on the pair kernel (skew_dims)
    const bool pair_tail = !halo && left > tail && pair_tail_on(h);
    struct TailFlag {
        golhip_t h;
        ~TailFlag() { h->pair_tail_step = false; }
    } tail_flag{h};
    h->pair_tail_step = pair_tail;
    while (left > tail) {
        if (!halo) {
            const int d = depth_plan(depth_cap(h, false), left - tail, pair_tail).d;
            if (int rc = launch_depth(h, d, left - d == 0, false)) return rc;
            left -= d;
            continue;
        }
        const HaloRun hr = halo_next(depth_cap(h, true), sched_rows(h), persist_on(h), left - tail);
        const int d = hr.d, k = hr.k;
        if (int rc = exchange_rccl(h, k * d, h->stream)) return rc;
        int prc = GOLHIP_OK;
        if (try_persist_halo(h, d, k, left - k * d == 0, &prc)) {
            left -= (int64_t)k * d;
            continue;
        }
        if (prc) return prc;
        for (int i = 0; i < k; ++i) {
            if (int rc = launch_ext(h, d, left - d == 0, (k - 1 - i) * d)) return rc;
            left -= d;
        }
    }
    if (want_flips && nturns > 0) {
        if (halo)
            if (int rc = exchange_rccl(h, 1, h->stream)) return rc;
        if (int rc = launch_depth(h, 1, true, halo)) return rc;
        if (int rc = start_flips(h)) return rc;
    }
    return GOLHIP_OK;
}

// golhip_step after its argument checks, with h->mu held: step_locked under
// the resident-launch guard (also each batch of golhip_view_stream).
int step_checked_locked(golhip_t h, int64_t nturns, int32_t want_flips) {
    if (!h->loaded) return fail(GOLHIP_EINVAL, "no board loaded");
    if (h->nranks == 1 && !h->torus()) return fail(GOLHIP_EINVAL, "strip handle needs golhip_comm_init or golhip_group_step");
    if (int rc = set_dev(h)) return rc;
    const int64_t turns0 = h->turns;
    const int cur0 = h->cur;
    // counters of this step, restored if a resident launch is abandoned below
    // (step_locked moves neither the flip nor the view counters; the
    // millisecond sums are not restored: drain_events may run meanwhile)
    const Counters n0 = h->n;
    const size_t ev0 = h->ev_pending.size();
    int rc = step_locked(h, nturns, want_flips);
    const bool light = h->guard_light;
    h->guard_light = false;
    if (rc || !h->guarded) {
        h->guarded = false;
        return rc;
    }
    // A resident launch ran (torus, or a one-rank ring): check it before returning.  Its
    // workgroups wait on their neighbours, so a co-tenant kernel holding CUs
    // can starve one past the bounded spin; then every workgroup drains out
    // with the error word set and the board is restored from the guard copy
    // (the board before this step) and re-run on the per-launch kernels.
    h->guarded = false;
    HIP_OR_FAIL(hipStreamSynchronize(h->stream));
    h->persist_pending = false;
    if (int rc_ = take_skew_err(h)) return rc_;
    if (!h->h_err || !*h->h_err) return GOLHIP_OK;  // (a one-rank ring's guard may see no resident launch)
    *h->h_err = 0;
    h->persistent = 0;  // this device is shared: no more resident launches on this handle
    h->persist_fallbacks++;
    h->n = n0;
    if (h->ev_pending.size() >= ev0) {  // the abandoned attempt's launch timings (unless drained meanwhile)
        for (size_t i = ev0; i < h->ev_pending.size(); ++i) {
            h->ev_pool.push_back(h->ev_pending[i].e0);
            h->ev_pool.push_back(h->ev_pending[i].e1);
        }
        h->ev_pending.resize(ev0);
    }
    if (!light)  // (a source-keeping launch left the step's board in buf[cur0])
        HIP_OR_FAIL(hipMemcpyAsync(h->buf[cur0] + (int64_t)kHalo * h->Ww, h->backup.p, (size_t)h->local_words() * 4,
                                   hipMemcpyDeviceToDevice, h->stream));
    h->cur = cur0;
    h->turns = turns0;
    h->alive_turn = -1;
    h->flips_valid = false;
    return step_locked(h, nturns, want_flips);
}

// golhip_group_step[_ex]: n strips (ring order = array order) driven from one
// process, halos moved by peer copies; want_flips keeps every strip's flip
// list of the last turn (golhip_flips, global coordinates, strip order =
// row-major order of the board).
// The strips of a group: one board, contiguous from row 0, covering it.
int group_check(golhip_t *hs, int32_t n, bool need_board) {
    if (!hs || n < 1) return fail(GOLHIP_EINVAL, "bad group");
    for (int i = 0; i < n; ++i) {
        if (int rc = check(hs[i])) return rc;
        if (need_board && !hs[i]->loaded) return fail(GOLHIP_EINVAL, "strip %d has no board", i);
        if (hs[i]->W != hs[0]->W || hs[i]->H != hs[0]->H || hs[i]->nranks != 1)
            return fail(GOLHIP_EINVAL, "strip %d does not belong to the group", i);
        if (hs[i]->birth != hs[0]->birth || hs[i]->survive != hs[0]->survive)
            return fail(GOLHIP_EINVAL, "strip %d has another rule than strip 0", i);
        if (hs[i]->plane != hs[0]->plane) return fail(GOLHIP_EINVAL, "strip %d has another topology than strip 0", i);
        const int expect_row0 = i == 0 ? 0 : hs[i - 1]->row0 + hs[i - 1]->rows;
        if (hs[i]->row0 != expect_row0) return fail(GOLHIP_EINVAL, "strip %d starts at %d, expected %d", i, hs[i]->row0, expect_row0);
    }
    if (hs[n - 1]->row0 + hs[n - 1]->rows != hs[0]->H) return fail(GOLHIP_EINVAL, "strips do not cover the board");
    return GOLHIP_OK;
}

// Halo rows of every strip from its ring neighbours' current boards: x rows
// each way (every strip's mutex held; ready: one event a strip).  relaunch:
// more than one launch follows the exchange (see below).
int group_exchange(golhip_t *hs, int32_t n, int x, hipEvent_t *ready, bool relaunch) {
    int rc = GOLHIP_OK;
    for (int i = 0; i < n && !rc; ++i) {
        HIP_RC(hipSetDevice(hs[i]->device));
        HIP_RC(hipEventRecord(ready[i], hs[i]->stream));
    }
    for (int i = 0; i < n && !rc; ++i) {
        golhip *me = hs[i], *prev = hs[(i - 1 + n) % n], *next = hs[(i + 1) % n];
        golhip_halo_plan_t p;
        halo_plan(me->rows, n, i, x, me->Ww, &p);
        HIP_RC(hipSetDevice(me->device));
        HIP_RC(hipStreamWaitEvent(me->stream, ready[(i - 1 + n) % n], 0));
        HIP_RC(hipStreamWaitEvent(me->stream, ready[(i + 1) % n], 0));
        const size_t bytes = (size_t)p.bytes;
        // top halo <- prev's last x rows; bottom halo <- next's first x rows
        uint32_t *mb = me->buf[me->cur];
        const uint32_t *pb = prev->buf[prev->cur] + (int64_t)(kHalo + prev->rows - x) * prev->Ww;
        const uint32_t *nb = next->buf[next->cur] + (int64_t)kHalo * next->Ww;
        HIP_RC(hipMemcpyPeerAsync(mb + (int64_t)p.recv_top_row * me->Ww, me->device, pb, prev->device, bytes,
                                  me->stream));
        HIP_RC(hipMemcpyPeerAsync(mb + (int64_t)p.recv_bottom_row * me->Ww, me->device, nb, next->device,
                                  bytes, me->stream));
        me->n.halo_bytes += 2 * (int64_t)bytes;
    }
    // a strip's second launch rewrites the buffer its neighbours copied
    // from: every stream waits for its neighbours' copies first.  (One launch
    // an exchange writes the other buffer, and the next exchange's first
    // waits order the launch after it behind these copies.)
    for (int i = 0; i < n && !rc && relaunch; ++i) {
        HIP_RC(hipSetDevice(hs[i]->device));
        HIP_RC(hipEventRecord(ready[i], hs[i]->stream));
    }
    for (int i = 0; i < n && !rc && relaunch; ++i) {
        HIP_RC(hipSetDevice(hs[i]->device));
        HIP_RC(hipStreamWaitEvent(hs[i]->stream, ready[(i - 1 + n) % n], 0));
        HIP_RC(hipStreamWaitEvent(hs[i]->stream, ready[(i + 1) % n], 0));
    }
    return rc;
}

// The rounds of a group step over the strips ss: per round one deep-halo
// exchange of k d rows and k launches of d turns, launch j over the rows
// [-ext, rows + ext), ext = (k - 1 - j) d (a lone strip: torus launches, no
// exchange).  owners: ss are the wide strips of these (padded strips,
// golhip_pad.cpp), and every launch follows a seam refresh of the rows it reads.
int group_rounds(golhip_t *ss, golhip_t *owners, int32_t n, int64_t turns, bool count_last, hipEvent_t *ready) {
    int rc = GOLHIP_OK;
    int64_t left = turns;
    while (left > 0 && rc == GOLHIP_OK) {
        int cap = GOLHIP_MAX_TB_DEPTH;
        for (int i = 0; i < n; ++i) cap = std::min(cap, depth_cap(ss[i], n > 1));
        const DepthRun run = depth_plan(cap, left);
        const int d = run.d;
        int k = 1;
        if (n > 1) {
            k = kHalo / d;
            for (int i = 0; i < n; ++i) k = std::min(k, halo_launches(ss[i]->rows, d, run.n));
            rc = group_exchange(ss, n, k * d, ready);
        }
        for (int j = 0; j < k && rc == GOLHIP_OK; ++j) {
            const int ext = (k - 1 - j) * d;
            const bool count = count_last && left - d == 0;
            for (int i = 0; i < n && !rc; ++i) {
                HIP_RC(hipSetDevice(ss[i]->device));
                if (rc) break;
                // a wide strip: the rows this launch reads (a lone strip is a torus: its own rows)
                if (owners)
                    rc = n > 1 ? pad_seam(owners[i], -(ext + d), ss[i]->rows + ext + d)
                               : pad_seam(owners[i], 0, ss[i]->rows);
                if (rc) break;
                rc = n > 1 ? launch_ext(ss[i], d, count, ext) : launch_depth(ss[i], d, count, false);
            }
            left -= d;
        }
    }
    return rc;
}

// The step of a checked group with every strip's mutex held.  `keep`
// (golhip_group_view_stream): the caller's n events, left alive, and no
// synchronisation at the end: the caller synchronises every stream and takes
// the skew flags itself.
int group_step_locked(golhip_t *hs, int32_t n, int64_t nturns, int32_t want_flips, hipEvent_t *keep, bool pad) {
    std::vector<hipEvent_t> ready(n, nullptr);
    int rc = GOLHIP_OK;
    for (int i = 0; i < n; ++i) {
        HIP_RC(hipSetDevice(hs[i]->device));
        if (keep)
            ready[i] = keep[i];
        else
            HIP_RC(hipEventCreateWithFlags(&ready[i], hipEventDisableTiming));
        if (!rc && want_il(hs[i]) != want_il(hs[0])) rc = fail(GOLHIP_EINVAL, "strip %d uses another word layout", i);
        if (!rc) rc = set_layout(hs[i], want_il(hs[i]));
        hs[i]->flips_valid = false;
    }
    auto exchange = [&](int x) {
        if (!rc) rc = group_exchange(hs, n, x, ready.data());
    };
    const int64_t tail = (want_flips && nturns > 0) ? 1 : 0;
    int64_t left = nturns - tail;
    if (!rc && pad && pad_group_wanted(hs, n, left)) {
        // a width that is no multiple of 32 on the fast kernels, as padded strips
        // (golhip_pad.cpp); the last turn of a want_flips step runs on K1g below
        bool ran = false;
        rc = pad_group_step(hs, n, left, ready.data(), &ran);
        if (ran) left = 0;
    }
    if (!rc && left > 0) rc = group_rounds(hs, nullptr, n, left, true, ready.data());
    if (tail && rc == GOLHIP_OK) {  // the last turn alone, then its flip list on every strip
        if (n > 1) exchange(1);
        for (int i = 0; i < n && !rc; ++i) {
            HIP_RC(hipSetDevice(hs[i]->device));
            if (!rc) rc = n > 1 ? launch_ext(hs[i], 1, true, 0) : launch_depth(hs[i], 1, true, false);
            if (!rc) rc = start_flips(hs[i]);
        }
    }
    for (int i = 0; i < n && !keep; ++i) {
        HIP_RC(hipSetDevice(hs[i]->device));
        if (ready[i]) {
            HIP_RC(hipStreamSynchronize(hs[i]->stream));
            HIP_RC(hipEventDestroy(ready[i]));
        }
        if (!rc) rc = take_skew_err(hs[i]);
    }
    return rc;
}

static int group_step_impl(golhip_t *hs, int32_t n, int64_t nturns, int32_t want_flips) {
    if (nturns < 0) return fail(GOLHIP_EINVAL, "bad group");
    if (int rc = group_check(hs, n)) return rc;
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    return group_step_locked(hs, n, nturns, want_flips);
}

}  // namespace gh

using namespace gh;

extern "C" {

int golhip_step(golhip_t h, int64_t nturns, int32_t want_flips) {
    if (int rc = check(h)) return rc;
    if (nturns < 0) return fail(GOLHIP_EINVAL, "nturns %lld", (long long)nturns);
    std::lock_guard<std::mutex> g(h->mu);
    return step_checked_locked(h, nturns, want_flips);
}

int golhip_comm_unique_id(uint8_t id[GOLHIP_UNIQUE_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == GOLHIP_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!id) return fail(GOLHIP_EINVAL, "id is null");
    ncclUniqueId u;
    NCCL_OR_FAIL(ncclGetUniqueId(&u));
    memcpy(id, &u, sizeof u);
    return GOLHIP_OK;
}

int golhip_comm_init(golhip_t h, const uint8_t id[GOLHIP_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank) {
    if (int rc = check(h)) return rc;
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail(GOLHIP_EINVAL, "rank %d of %d", rank, nranks);
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    if (h->ringed()) return fail(GOLHIP_EINVAL, "comm already initialised");
    if (!h->conway()) return fail(GOLHIP_EINVAL, "a ring runs Conway's B3/S23 only: this handle has another rule (golhip_set_rule)");
    if (h->plane) return fail(GOLHIP_EINVAL, "a ring runs the torus only: this handle is a bounded plane (golhip_set_topology)");
    if (nranks > 1 && h->rows < 1) return fail(GOLHIP_EINVAL, "empty strip");
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    NCCL_OR_FAIL(ncclCommInitRank(&h->comm, nranks, u, rank));
    h->nranks = nranks;
    h->rank = rank;
    // agree on the schedule: the smallest strip of the ring
    int32_t *d_rows = nullptr;
    HIP_OR_FAIL(hipMalloc(&d_rows, sizeof(int32_t)));
    int32_t rows = h->rows;
    hipError_t e = hipMemcpyAsync(d_rows, &rows, sizeof rows, hipMemcpyHostToDevice, h->stream);
    ncclResult_t nr = e == hipSuccess ? ncclAllReduce(d_rows, d_rows, 1, ncclInt32, ncclMin, h->comm, h->stream) : ncclSuccess;
    if (e == hipSuccess && nr == ncclSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess && nr == ncclSuccess) e = hipMemcpy(&rows, d_rows, sizeof rows, hipMemcpyDeviceToHost);
    (void)hipFree(d_rows);
    if (nr != ncclSuccess) return fail(GOLHIP_ERCCL, "ncclAllReduce(strip rows): %s", ncclGetErrorString(nr));
    if (e != hipSuccess) return fail(GOLHIP_EHIP, "strip rows: %s", hipGetErrorString(e));
    h->ring_rows = rows;
    return GOLHIP_OK;
}

int golhip_test_ring_init(golhip_t h, int32_t nranks, int32_t rank, int32_t ring_rows, golhip_test_transport_fn fn,
                          void *user) {
    if (int rc = check(h)) return rc;
    if (!test_hooks_env()) return fail(GOLHIP_EINVAL, "golhip_test_ring_init is a test hook: set GOLHIP_TEST_HOOKS=1");
    if (!fn || nranks < 1 || rank < 0 || rank >= nranks) return fail(GOLHIP_EINVAL, "rank %d of %d", rank, nranks);
    std::lock_guard<std::mutex> g(h->mu);
    if (h->ringed()) return fail(GOLHIP_EINVAL, "comm already initialised");
    if (!h->conway()) return fail(GOLHIP_EINVAL, "a ring runs Conway's B3/S23 only: this handle has another rule (golhip_set_rule)");
    if (h->plane) return fail(GOLHIP_EINVAL, "a ring runs the torus only: this handle is a bounded plane (golhip_set_topology)");
    if (!h->strip || h->rows < 1 || ring_rows < 1 || ring_rows > h->rows)
        return fail(GOLHIP_EINVAL, "a strip handle and 1 <= ring_rows <= its rows");
    h->xport = fn;
    h->xport_user = user;
    h->nranks = nranks;
    h->rank = rank;
    h->ring_rows = ring_rows;
    return GOLHIP_OK;
}

int golhip_comm_info(golhip_t h, int32_t *nranks, int32_t *rank, int32_t *ring_rows) {
    if (int rc = check(h)) return rc;
    if (!nranks || !rank || !ring_rows) return fail(GOLHIP_EINVAL, "null output");
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->comm) {  // no ring: this handle alone (or the test transport's ring)
        *nranks = h->xport ? h->nranks : 1;
        *rank = h->xport ? h->rank : 0;
        *ring_rows = h->xport ? h->ring_rows : h->rows;
        return GOLHIP_OK;
    }
    int n = 0, r = 0;
    NCCL_OR_FAIL(ncclCommCount(h->comm, &n));
    NCCL_OR_FAIL(ncclCommUserRank(h->comm, &r));
    *nranks = n;
    *rank = r;
    *ring_rows = h->ring_rows;
    return GOLHIP_OK;
}

int golhip_group_step(golhip_t *hs, int32_t n, int64_t nturns) { return group_step_impl(hs, n, nturns, 0); }

int golhip_group_step_ex(golhip_t *hs, int32_t n, int64_t nturns, int32_t want_flips) {
    return group_step_impl(hs, n, nturns, want_flips);
}

}  // extern "C"
