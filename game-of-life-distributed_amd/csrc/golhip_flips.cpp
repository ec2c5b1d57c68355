// golhip_flips.cpp — flip lists: the three-pass compaction (golhip_flips,
// golhip_alive_cells), the flip stream (K5 per turn, K5r resident) and the
// stream of a group of row strips (K5 per strip and turn, one gather a strip).
#include "golhip_impl.h"
#include "gol_flip_merge.h"
#include <climits>
#include <cstdlib>

namespace gh GOLHIP_HIDDEN {

// K5r (flip_overlap 2): copy blocks of the resident flip-stream launch
static constexpr int kFlipStreamCopyBlocks = 128;
static constexpr int64_t kFlipStreamMinBlocks = 64;  // (64 K words, e.g. 1448^2)

// Count and scan of the flip list (current against previous board) into d_blk
// and d_scalars[1]: what finish_compact scatters from.
static int count_flips(golhip_t h) {
    const int64_t nw = h->local_words();
    const int64_t nb = golk::compact_blocks(nw);
    int rc = h->d_blk.ensure(h, nb);
    if (rc) return rc;
    HIP_OR_FAIL(golk::launch_compact_count(h->cur_rows(), h->prev_rows(), nw, h->d_blk.p, h->stream));
    HIP_OR_FAIL(golk::launch_compact_scan(h->d_blk.p, nb, h->d_scalars + 1, h->stream));
    h->flips_counted = true;
    return GOLHIP_OK;
}

int start_flips(golhip_t h) {
    if (int rc = count_flips(h)) return rc;
    h->flips_valid = true;
    h->flips_turn = h->turns;
    return GOLHIP_OK;
}

// Room for n (x, y) pairs in d_xy (at least 4096).
static int ensure_xy(golhip_t h, int64_t n) { return h->d_xy.ensure(h, 2 * n, false, 2 * 4096); }

// Finish a compaction started with count+scan: read the total, scatter, copy out.
static int finish_compact(golhip_t h, const uint32_t *a, const uint32_t *b, int32_t *xy, uint64_t cap, uint64_t *n) {
    HIP_OR_FAIL(hipMemcpyAsync(h->h_scalars + 1, h->d_scalars + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               h->stream));
    if (int rc_ = sync_stream(h)) return rc_;
    const uint64_t total = h->h_scalars[1];
    if (n) *n = total;
    if (total > cap || (!xy && total > 0))
        return fail(GOLHIP_ERANGE, "buffer holds %llu cells, %llu needed", (unsigned long long)cap,
                    (unsigned long long)total);
    if (total == 0) return GOLHIP_OK;
    int rc = ensure_xy(h, (int64_t)total);
    if (rc) return rc;
    HIP_OR_FAIL(golk::launch_compact_scatter(a, b, h->local_words(), h->Ww, h->row0, h->d_blk.p, h->d_xy.p, h->il, h->stream));
    HIP_OR_FAIL(hipMemcpyAsync(xy, h->d_xy.p, total * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (int rc_ = sync_stream(h)) return rc_;
    return GOLHIP_OK;
}

// One batch of the flip stream: the caller's request and what its paths share.
struct FlipBatch {
    int64_t nturns;
    int format;
    void *out;
    uint64_t cap;
    uint64_t *counts;
    bool stop;
    bool halo;       // the turns exchange a halo row first (golhip::halo_mode)
    int esz;         // bytes an entry
    int64_t nw;      // words of this handle's rows
    uint64_t dcap;   // entries the lists can take: cap, or all a batch can ever hold
    std::vector<unsigned long long> run;  // running list offsets, one more than turns
    // K5 / K5r
    void *direct;        // device address of `out` in golhip_host_alloc memory, or null
    int64_t nb;          // compute blocks of a turn
    int64_t nlaunch;     // turns launched
    bool coresident;
    golk::StepArgs sa;
};

// Giant strips (2^32 - 4096 words or more, past K5's 32-bit word index) and
// handles with another rule than Conway's (K5 / K5r are B3/S23): one
// per-launch turn and the three-pass compaction at a time, checked on the
// host after each turn.
static int flip_generic(golhip_t h, FlipBatch &b, int64_t *done_out, uint64_t *total_out) {
    const int64_t nw = b.nw, nturns = b.nturns;
    const uint64_t dcap = b.dcap;
    std::vector<unsigned long long> &run = b.run;
    const int64_t nb = golk::compact_blocks(nw);
    if (int rc = h->d_blk.ensure(h, nb)) return rc;
    if (int rc = ensure_xy(h, (int64_t)std::min<uint64_t>(dcap, (uint64_t)nw * 32))) return rc;
    if (int rc = set_layout(h, want_il(h))) return rc;
    std::vector<int32_t> xy;
    int64_t t = 0;
    for (; t < nturns; ++t) {
        if (b.halo)
            if (int rc = exchange_rccl(h, 1, h->stream)) return rc;
        if (int rc = launch_depth(h, 1, t == nturns - 1, b.halo)) return rc;
        HIP_OR_FAIL(golk::launch_compact_count(h->cur_rows(), h->prev_rows(), nw, h->d_blk.p, h->stream));
        HIP_OR_FAIL(golk::launch_compact_scan(h->d_blk.p, nb, h->d_scalars + 1, h->stream));
        HIP_OR_FAIL(hipMemcpyAsync(h->h_scalars + 1, h->d_scalars + 1, 8, hipMemcpyDeviceToHost, h->stream));
        if (int rc = sync_stream(h)) return rc;
        const uint64_t k = h->h_scalars[1];
        if (b.stop && run[t] + k > dcap) {  // roll back this turn
            h->cur ^= 1;
            h->turns -= 1;
            h->alive_turn = -1;
            run[t + 1] = run[t] + k;
            break;
        }
        run[t + 1] = run[t] + k;
        const uint64_t keep = run[t] >= dcap ? 0 : std::min<uint64_t>(k, dcap - run[t]);
        if (keep > 0) {
            HIP_OR_FAIL(golk::launch_compact_scatter(h->cur_rows(), h->prev_rows(), nw, h->Ww, h->row0, h->d_blk.p,
                                                     h->d_xy.p, h->il, h->stream, (unsigned long long)(h->d_xy.cap / 2)));
            xy.resize(2 * keep);
            HIP_OR_FAIL(hipMemcpyAsync(xy.data(), h->d_xy.p, keep * 8, hipMemcpyDeviceToHost, h->stream));
            if (int rc = sync_stream(h)) return rc;
            for (uint64_t e = 0; e < keep; ++e) {
                if (b.format == GOLHIP_FLIPS_XY) {
                    static_cast<int32_t *>(b.out)[2 * (run[t] + e)] = xy[2 * e];
                    static_cast<int32_t *>(b.out)[2 * (run[t] + e) + 1] = xy[2 * e + 1];
                } else {
                    static_cast<uint32_t *>(b.out)[run[t] + e] =
                        (uint32_t)((uint64_t)xy[2 * e + 1] * (uint64_t)h->W + (uint64_t)xy[2 * e]);
                }
            }
        }
    }
    const int64_t done = t;
    for (int64_t i = 0; i < done; ++i) b.counts[i] = run[i + 1] - run[i];
    *done_out = done;
    *total_out = (b.stop && done < nturns) ? (done == 0 ? run[1] : run[done]) : run[done];
    return GOLHIP_OK;
}

// The FlipTurnArgs fields every launch of a batch sets alike: those of a
// copy-only launch, and (compute) those of a launch that also steps a turn.
static golk::FlipTurnArgs flip_turn_args(golhip_t h, const FlipBatch &b, bool compute) {
    golk::FlipTurnArgs a{};
    a.Ww = h->Ww;
    a.format = b.format == GOLHIP_FLIPS_XY ? golk::kFlipFormatXY : golk::kFlipFormatIdx;
    a.cap = b.dcap;
    a.ctl = h->d_ftctl.p;
    a.stop_on_overflow = b.stop ? 1 : 0;
    if (!compute) return a;
    a.W = h->W;
    a.rows = h->rows;
    a.dst_base = kHalo;
    a.in = b.sa.in;
    a.row0 = h->row0;
    a.ncompute = (int)b.nb;
    a.status = h->d_ftstatus.p;
    a.dbg = h->flip_debug;
    return a;
}

// K5r: the whole batch in one launch (see FlipStreamArgs) whose `ncopy` copy
// blocks move each turn's list to the host while the next turns compute.
static int flip_resident_batch(golhip_t h, const FlipBatch &b, int ncopy, uint64_t board_bytes) {
    const int64_t nlaunch = b.nlaunch;
    // per turn kFtShards counters 128 B apart, then one turn count per compute block
    const int64_t ndone = nlaunch * golk::kFtShards * golk::kFtShardStride + b.nb;
    if (int rc = h->d_ftdone.ensure(h, ndone)) return rc;
    HIP_OR_FAIL(hipMemsetAsync(h->d_ftdone.p, 0, (size_t)ndone * sizeof(unsigned), h->stream));
    HIP_OR_FAIL(hipMemsetAsync(h->d_scalars, 0, sizeof(unsigned long long), h->stream));
    golk::FlipStreamArgs fs{};
    fs.turn = flip_turn_args(h, b, true);
    fs.turn.out = h->d_ev.p;
    fs.turn.coresident = 1;
    fs.turn.board_bytes = (unsigned)board_bytes;
    fs.turn.out_bytes = (unsigned)((uint64_t)b.dcap * b.esz);
    fs.buf0 = h->buf[0];
    fs.buf1 = h->buf[1];
    fs.first = h->cur;
    fs.nturns = (int)nlaunch;
    // turn t's epoch is epoch0 + t: never 0 (the zeroed status words) in the batch
    if (((h->flip_epoch + 1) & 0x3FFFFFu) + (unsigned)nlaunch > 0x3FFFFFu) h->flip_epoch = 0;
    fs.epoch0 = (h->flip_epoch + 1) & 0x3FFFFFu;
    h->flip_epoch = (fs.epoch0 + (unsigned)nlaunch - 1) & 0x3FFFFFu;
    fs.run = h->d_run.p;
    fs.done = h->d_ftdone.p;
    fs.blk_done = h->d_ftdone.p + nlaunch * golk::kFtShards * golk::kFtShardStride;
    fs.alive = h->d_scalars;
    fs.cp_dst = b.direct;
    fs.ncopy = ncopy;
    fs.cp_groups = std::max(1, std::min(h->flip_cp_groups, ncopy / 8));
    fs.timeout_ticks = 200000000ll;  // 2 s: only a block that never became resident waits that long
    if (int rc = span_begin(h, h->stream)) return rc;
    HIP_OR_FAIL(golk::launch_flip_stream(fs, h->stream));
    if (int rc = span_end(h, 2)) return rc;
    h->n.flip_launches += nlaunch;
    h->n.flip_resident++;
    h->cur ^= (int)(nlaunch & 1);
    h->turns += nlaunch;
    return GOLHIP_OK;
}

// Turn t of a batch: one K5 launch (the halo rows, if used, already in place).
static int flip_turn_launch(golhip_t h, const FlipBatch &b, int64_t t, bool overlap, int cpb) {
    const bool last = t == b.nlaunch - 1;
    if (last) HIP_OR_FAIL(hipMemsetAsync(h->d_scalars, 0, sizeof(unsigned long long), h->stream));
    golk::FlipTurnArgs a = flip_turn_args(h, b, true);
    a.src = h->buf[h->cur];
    a.dst = h->buf[h->cur ^ 1];
    a.out = b.direct && !overlap ? b.direct : (void *)h->d_ev.p;
    a.cp_run = overlap && t > 0 ? h->d_run.p + t - 1 : nullptr;
    a.cp_dst = b.direct;
    a.cp_blocks = cpb;
    a.run = h->d_run.p + t;
    a.ticket = h->d_ftticket.p + t;
    h->flip_epoch = (h->flip_epoch + 1) & 0x3FFFFFu;
    if (h->flip_epoch == 0) h->flip_epoch = 1;  // 0 is the zeroed status array's epoch
    a.epoch = h->flip_epoch;
    a.coresident = b.coresident ? 1 : 0;
    a.alive = last ? h->d_scalars : nullptr;
    if (int rc = span_begin(h, h->stream)) return rc;
    if (h->rule_path())  // (here only with golhip_set_rule_flips 1: K14)
        HIP_OR_FAIL(golk::launch_rule_flip_turn(a, h->birth, h->survive, h->rule_kernel == 2, h->stream));
    else
        HIP_OR_FAIL(golk::launch_flip_turn(a, h->stream));
    if (int rc = span_end(h, 2)) return rc;
    h->n.flip_launches++;
    h->cur ^= 1;
    h->turns += 1;
    return GOLHIP_OK;
}

// One K5 launch per turn.  overlap (flip_overlap 1): each launch's `cpb` copy
// blocks move the previous turn's list to the host, and a copy-only launch
// the last turn's; else the turn's own blocks store into `out` (direct) or d_ev.
static int flip_turn_loop(golhip_t h, const FlipBatch &b, bool overlap, int cpb) {
    for (int64_t t = 0; t < b.nlaunch; ++t) {
        if (b.halo)
            if (int rc = exchange_rccl(h, 1, h->stream)) return rc;
        if (int rc = flip_turn_launch(h, b, t, overlap, cpb)) return rc;
    }
    if (overlap && b.nlaunch > 0) {  // the last turn's list: a copy-only launch
        golk::FlipTurnArgs a = flip_turn_args(h, b, false);
        a.out = h->d_ev.p;
        a.ncompute = 0;
        a.cp_run = h->d_run.p + b.nlaunch - 1;
        a.cp_dst = b.direct;
        a.cp_blocks = 256;
        if (int rc = span_begin(h, h->stream)) return rc;
        HIP_OR_FAIL(golk::launch_flip_turn(a, h->stream));
        if (int rc = span_end(h, 2)) return rc;
    }
    return GOLHIP_OK;
}

// The CellFlipped stream (distributor.go:93-173 with initializeAliveCells,
// :212-220): up to nturns single turns, each with its flip list appended in
// turn order to `out` (row-major within a turn; format: int32 (x, y) pairs or
// uint32 y * W + x).  stop: never lose an entry — the batch ends before the
// first turn whose list would not fit (the board is left at the last turn
// that did, *done says which); otherwise the board advances nturns and the
// lists are cut at cap (*total is what they needed).  counts[t] = entries
// of turn t, for t < *done.
static int flip_stream_locked(golhip_t h, int64_t nturns, int format, void *out, uint64_t cap, uint64_t *counts,
                              int64_t *done_out, uint64_t *total_out, bool stop) {
    *done_out = 0;
    *total_out = 0;
    if (!h->loaded) return fail(GOLHIP_EINVAL, "no board loaded");
    if (h->nranks == 1 && !h->torus()) return fail(GOLHIP_EINVAL, "strip handle needs golhip_comm_init");
    if (int rc = set_dev(h)) return rc;
    h->flips_valid = false;
    if (nturns == 0) return GOLHIP_OK;
    FlipBatch b{};
    b.nturns = nturns;
    b.format = format;
    b.out = out;
    b.cap = cap;
    b.counts = counts;
    b.stop = stop;
    b.halo = h->halo_mode();
    const int esz = b.esz = format == GOLHIP_FLIPS_XY ? 8 : 4;
    const int64_t nw = b.nw = h->local_words();
    const uint64_t most = (uint64_t)nturns * (uint64_t)h->W * (uint64_t)h->rows;
    const uint64_t dcap = b.dcap = std::min<uint64_t>({cap, most, (uint64_t)INT64_MAX / 16});
    if (int rc = h->d_run.ensure(h, nturns + 1)) return rc;
    b.run.assign((size_t)nturns + 1, 0);
    std::vector<unsigned long long> &run = b.run;
    unsigned ctl[2] = {0, 0};
    const int64_t t0 = h->turns;
    const int c0 = h->cur;

    if (nw >= (1ll << 32) - 4096 || !h->fused_flips()) return flip_generic(h, b, done_out, total_out);
    // a rule handle here (golhip_set_rule_flips 1) runs K14, K5's per-launch kernel with the rule as a
    // policy: everything below holds for it, with its own occupancy and no resident form
    const bool k14 = h->rule_path();

    // fused turn + list (K5) on the canonical layout, at any width (W % 32 != 0:
    // the kernel closes the row seam itself, no padded torus); into a golhip_host_alloc
    // buffer the entries go without a host-side copy (option "flip_overlap"):
    //  2: K5r, the batch's turns in one resident launch whose copy blocks
    //     move each turn's list to the host while the next turns compute
    //     (round 6; where it cannot run: 1);
    //  1: each K5 launch's copy blocks move the previous turn's list;
    //  0: the turn's own blocks store their entries there directly
    if (int rc = set_layout(h, 0)) return rc;
    void *direct = b.direct = mapped_device_ptr(out, (size_t)dcap * esz);
    const int64_t nb = b.nb = golk::flip_turn_blocks(nw);
    const bool contig = h->Ww % 4 == 0;
    const int bpc = std::min(k14 ? golk::rule_flip_turn_blocks_per_cu(contig, h->W % 32 != 0, h->birth, h->survive,
                                                                      h->rule_kernel == 2)
                                 : golk::flip_turn_blocks_per_cu(contig, h->W % 32 != 0),
                             4);
    // every block resident at once (with a 10 % margin): block order = blockIdx.
    // Not in a multi-rank ring: its fallback (restore, re-run in ticket order)
    // would redo the batch's exchanges on this rank alone and hang the ring.
    const bool coresident = b.coresident = !h->ft_ticket && !(h->ringed() && h->nranks > 1) && bpc > 0 &&
                                           nb * 10 <= (int64_t)h->cu_count * bpc * 9;
    // K5r: copy blocks in the slots the turn's blocks leave (up to 128), every
    // block resident; whole tori (a strip exchanges halos between turns);
    // buffers its 32-bit buffer offsets reach
    const int ncopy_r = (int)std::min<int64_t>(kFlipStreamCopyBlocks, (int64_t)h->cu_count * std::max(bpc, 1) - nb);
    const uint64_t board_bytes = (uint64_t)h->phys_rows * h->Ww * 4;
    // (A/B of handles a caller creates itself, e.g. the gol.Run mirror's:
    // GOLHIP_TUNING=1 GOLHIP_FLIP_OVERLAP=n overrides the option)
    if (const char *e = getenv("GOLHIP_FLIP_OVERLAP"); e && tuning_env() && e[0] >= '0' && e[0] <= '3' && !e[1])
        h->flip_overlap = e[0] - '0';
    if (const char *e = getenv("GOLHIP_FLIP_CP_GROUPS"); e && tuning_env() && e[0] >= '1' && e[0] <= '8' && !e[1])
        h->flip_cp_groups = e[0] - '0';
    // (boards under kFlipStreamMinBlocks blocks keep per-turn launches: their
    // lists are short, and K5r's per-turn waits cost more than a launch;
    // configs[0] through gol.Run measured within noise, profiles/r7u)
    const bool resident = !k14 && direct && (h->flip_overlap == 3 || (h->flip_overlap == 2 && nb >= kFlipStreamMinBlocks)) &&
                          coresident && !b.halo && ncopy_r >= 8 &&
                          board_bytes < (1ull << 31) && (uint64_t)dcap * esz < (1ull << 31);
    const int ov = !direct ? 0 : resident ? 2 : std::min(h->flip_overlap, 1);
    const bool overlap = ov == 1;
    // launch the turns the buffer probably holds (the last batch's largest
    // list); turns past an overflow would only return at once
    int64_t nlaunch = nturns;
    if (stop && h->ft_est > 0) nlaunch = std::min<int64_t>(nturns, (int64_t)(dcap / h->ft_est) + 1);
    b.nlaunch = nlaunch;
    if (int rc = h->d_ftstatus.ensure(h, 3 * nb, true)) return rc;  // (K5r: three sets)
    if (int rc = h->d_ftticket.ensure(h, nlaunch)) return rc;
    if (int rc = h->d_ftctl.ensure(h, 2)) return rc;
    if (!direct || ov)
        if (int rc = h->d_ev.ensure(h, (int64_t)std::max<uint64_t>(dcap, 1) * esz)) return rc;
    if (coresident) {  // keep the batch recoverable (see the error check below)
        if (int rc = h->backup.ensure(h, h->local_words())) return rc;
        HIP_OR_FAIL(hipMemcpyAsync(h->backup.p, h->cur_rows(), (size_t)h->local_words() * 4, hipMemcpyDeviceToDevice,
                                   h->stream));
    }
    // every run bound zeroed: a turn that never ran (after a stop) reads as an
    // empty list to the next launch's copy blocks
    HIP_OR_FAIL(hipMemsetAsync(h->d_run.p, 0, (size_t)(nlaunch + 1) * sizeof(unsigned long long), h->stream));
    // copy blocks: the slots the turn's blocks leave free (they come after
    // them in the grid, so the turn's blocks stay co-resident), 32..256
    const int cpb = overlap ? (int)std::max<int64_t>(32, std::min<int64_t>(256, (int64_t)h->cu_count * std::max(bpc, 1) - nb))
                            : 0;
    HIP_OR_FAIL(hipMemsetAsync(h->d_ftticket.p, 0, (size_t)nlaunch * sizeof(unsigned), h->stream));
    HIP_OR_FAIL(hipMemsetAsync(h->d_ftctl.p, 0, 2 * sizeof(unsigned), h->stream));
    b.sa = step_args(h, nullptr, b.halo);
    if (ov == 2) {
        if (nlaunch > 0)
            if (int rc = flip_resident_batch(h, b, ncopy_r, board_bytes)) return rc;
    } else if (int rc = flip_turn_loop(h, b, overlap, cpb)) {
        return rc;
    }
    HIP_OR_FAIL(hipMemcpyAsync(run.data(), h->d_run.p, (size_t)(nlaunch + 1) * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, h->stream));
    HIP_OR_FAIL(hipMemcpyAsync(ctl, h->d_ftctl.p, sizeof ctl, hipMemcpyDeviceToHost, h->stream));
    if (int rc = sync_stream(h)) return rc;
    for (auto &r : run) r &= ~golk::kFtRunReady;  // (K5r's ready bit)
    if (ctl[1]) {
        if (!coresident) return fail(GOLHIP_EHIP, "flip stream: look-back spin bound exceeded (board undefined)");
        // a block waited on a predecessor that never ran (a co-tenant kernel
        // held CUs): restore the batch's first board, re-run it in ticket order
        HIP_OR_FAIL(hipMemcpyAsync(h->buf[c0] + (int64_t)kHalo * h->Ww, h->backup.p, (size_t)h->local_words() * 4,
                                   hipMemcpyDeviceToDevice, h->stream));
        h->cur = c0;
        h->turns = t0;
        h->alive_turn = -1;
        h->ft_ticket = true;
        h->flip_fallbacks++;
        h->flip_debug &= ~4;
        return flip_stream_locked(h, nturns, format, out, cap, counts, done_out, total_out, stop);
    }
    int64_t done = nlaunch;
    if (stop)
        for (int64_t t = 0; t < nlaunch; ++t)
            if (run[t + 1] > dcap) {
                done = t;
                break;
            }
    if (done < nlaunch) {  // turn `done` overflowed and the later launches returned at once
        h->cur = (c0 + (int)(done & 1)) & 1;
        h->turns = t0 + done;
        h->alive_turn = -1;
    } else {
        h->alive_turn = h->turns;
    }
    uint64_t most_one = 0;
    for (int64_t t = 0; t < done; ++t) {
        counts[t] = run[t + 1] - run[t];
        most_one = std::max<uint64_t>(most_one, counts[t]);
    }
    if (done > 0) h->ft_est = most_one;
    const uint64_t total = done < nlaunch ? (done == 0 ? run[1] : run[done]) : run[nlaunch];
    const uint64_t got = done == 0 && stop ? 0 : std::min<uint64_t>(run[done], cap);
    if (got > 0 && !direct) {
        HIP_OR_FAIL(hipMemcpyAsync(out, h->d_ev.p, got * esz, hipMemcpyDeviceToHost, h->stream));
        if (int rc = sync_stream(h)) return rc;
    }
    h->n.flip_entries += (int64_t)got;
    *done_out = done;
    *total_out = total;
    return GOLHIP_OK;
}

// ---- golhip_group_flip_stream: the stream of a board held as row strips ----

// One entry of the caller's list from an (x, y) pair.
static inline void put_entry(void *out, int format, uint64_t at, int32_t x, int32_t y, int W) {
    if (format == GOLHIP_FLIPS_XY) {
        static_cast<int32_t *>(out)[2 * at] = x;
        static_cast<int32_t *>(out)[2 * at + 1] = y;
    } else {
        static_cast<uint32_t *>(out)[at] = (uint32_t)((uint64_t)y * (uint64_t)W + (uint64_t)x);
    }
}

static int group_sync(golhip_t *hs, int n) {
    for (int i = 0; i < n; ++i) {
        if (int rc = set_dev(hs[i])) return rc;
        if (int rc = sync_stream(hs[i])) return rc;
    }
    return GOLHIP_OK;
}

// Giant strips (2^32 - 4096 words or more) and groups with another rule than
// Conway's: one group turn at a time through
// the three-pass compaction, the board's count checked on the host before the
// turn's entries are fetched (two synchronisations a turn); a turn that does
// not fit is undone on every strip (its source board is still the other buffer).
static int group_flip_generic(golhip_t *hs, int n, int64_t nturns, int format, void *out, uint64_t cap, uint64_t *counts,
                              hipEvent_t *ready, int64_t *done_out, uint64_t *total_out) {
    std::vector<std::vector<int32_t>> xy((size_t)n);
    std::vector<uint64_t> k((size_t)n);
    uint64_t acc = 0, need = 0;
    int64_t t = 0;
    for (; t < nturns; ++t) {
        if (int rc = group_step_locked(hs, n, 1, 1, ready)) return rc;
        for (int i = 0; i < n; ++i) {
            golhip *h = hs[i];
            if (int rc = set_dev(h)) return rc;
            HIP_OR_FAIL(hipMemcpyAsync(h->h_scalars + 1, h->d_scalars + 1, 8, hipMemcpyDeviceToHost, h->stream));
        }
        if (int rc = group_sync(hs, n)) return rc;
        uint64_t c = 0;
        for (int i = 0; i < n; ++i) c += k[i] = hs[i]->h_scalars[1];
        if (c > cap - acc) {
            for (int i = 0; i < n; ++i) {
                hs[i]->cur ^= 1;
                hs[i]->turns -= 1;
                hs[i]->alive_turn = -1;
                hs[i]->flips_valid = false;
            }
            need = c;
            break;
        }
        for (int i = 0; i < n; ++i) {
            golhip *h = hs[i];
            if (k[i] == 0) continue;
            if (int rc = set_dev(h)) return rc;
            if (int rc = ensure_xy(h, (int64_t)k[i])) return rc;
            HIP_OR_FAIL(golk::launch_compact_scatter(h->cur_rows(), h->prev_rows(), h->local_words(), h->Ww, h->row0,
                                                     h->d_blk.p, h->d_xy.p, h->il, h->stream));
            xy[i].resize(2 * k[i]);
            HIP_OR_FAIL(hipMemcpyAsync(xy[i].data(), h->d_xy.p, k[i] * 8, hipMemcpyDeviceToHost, h->stream));
        }
        if (int rc = group_sync(hs, n)) return rc;
        for (int i = 0; i < n; ++i) {
            for (uint64_t e = 0; e < k[i]; ++e) put_entry(out, format, acc + e, xy[i][2 * e], xy[i][2 * e + 1], hs[0]->W);
            acc += k[i];
            hs[i]->n.flip_entries += (int64_t)k[i];
        }
        counts[t] = c;
    }
    // the turns ran as steps that keep their list; a flip stream keeps none
    // (golhip_flips after it is GOLHIP_EINVAL, as after every other path of the stream)
    for (int i = 0; i < n; ++i) hs[i]->flips_valid = false;
    *done_out = t;
    *total_out = t == 0 ? need : acc;
    return GOLHIP_OK;
}

// Every width: per turn the group's 1-row halo exchange, then K5 on every
// strip's stream into the strip's own device list with its own running
// offsets (no strip waits for another's); nothing is synchronised in the turn
// loop.  Then the run arrays come back (first synchronisation), the merge
// plan (gol_flip_merge.h) places the segments, one gather launch a strip
// moves them into `out` (second synchronisation).  K5 runs in ticket order:
// strips that share a device share its CUs, so no strip's grid is known to
// be resident at once.
static int group_flip_fused(golhip_t *hs, int n, int64_t nturns, int format, void *out, uint64_t cap, uint64_t *counts,
                            hipEvent_t *ready, int64_t *done_out, uint64_t *total_out) {
    const int esz = format == GOLHIP_FLIPS_XY ? 8 : 4;
    golhip *g = hs[0];  // keeps the group's estimate and staging buffer
    // launch the turns the buffer certainly held at the last batch's largest
    // turn: a batch that stops early costs a restore and a re-run
    int64_t nlaunch = nturns;
    if (g->group_ft_est > 0) nlaunch = std::max<int64_t>(1, std::min<int64_t>(nturns, (int64_t)(cap / g->group_ft_est)));
    const int64_t t0 = g->turns;
    std::vector<FlipBatch> bs((size_t)n);
    std::vector<int> c0((size_t)n);
    for (int i = 0; i < n; ++i) {
        golhip *h = hs[i];
        if (int rc = set_dev(h)) return rc;
        if (int rc = set_layout(h, 0)) return rc;
        h->flips_valid = false;
        FlipBatch &b = bs[i];
        b.nturns = nturns;
        b.format = format;
        b.cap = cap;
        b.stop = true;
        b.esz = esz;
        b.nw = h->local_words();
        const uint64_t most = (uint64_t)nlaunch * (uint64_t)h->W * (uint64_t)h->rows;
        b.dcap = std::min<uint64_t>({cap, most, (uint64_t)INT64_MAX / 16});
        b.nb = golk::flip_turn_blocks(b.nw);
        b.nlaunch = nlaunch;
        b.coresident = false;
        b.sa = step_args(h, nullptr, n > 1);
        c0[i] = h->cur;
        if (int rc = h->d_run.ensure(h, nlaunch + 1)) return rc;
        if (int rc = h->d_goff.ensure(h, nlaunch)) return rc;
        if (int rc = h->d_ftstatus.ensure(h, 3 * b.nb, true)) return rc;
        if (int rc = h->d_ftticket.ensure(h, nlaunch)) return rc;
        if (int rc = h->d_ftctl.ensure(h, 2)) return rc;
        if (int rc = h->d_ev.ensure(h, (int64_t)std::max<uint64_t>(b.dcap, 1) * esz)) return rc;
        if (nlaunch > 1) {  // the board to restore when the batch stops early
            if (int rc = h->backup.ensure(h, h->local_words())) return rc;
            HIP_OR_FAIL(hipMemcpyAsync(h->backup.p, h->cur_rows(), (size_t)h->local_words() * 4, hipMemcpyDeviceToDevice,
                                       h->stream));
        }
        HIP_OR_FAIL(hipMemsetAsync(h->d_run.p, 0, (size_t)(nlaunch + 1) * sizeof(unsigned long long), h->stream));
        HIP_OR_FAIL(hipMemsetAsync(h->d_ftticket.p, 0, (size_t)nlaunch * sizeof(unsigned), h->stream));
        HIP_OR_FAIL(hipMemsetAsync(h->d_ftctl.p, 0, 2 * sizeof(unsigned), h->stream));
    }
    for (int64_t t = 0; t < nlaunch; ++t) {
        if (n > 1)
            if (int rc = group_exchange(hs, n, 1, ready, false)) return rc;
        for (int i = 0; i < n; ++i) {
            if (int rc = set_dev(hs[i])) return rc;
            if (int rc = flip_turn_launch(hs[i], bs[i], t, false, 0)) return rc;
        }
    }
    // first synchronisation: every strip's running offsets and flags
    std::vector<unsigned long long> runs((size_t)n * (size_t)(nlaunch + 1));
    std::vector<unsigned> ctl(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        golhip *h = hs[i];
        if (int rc = set_dev(h)) return rc;
        HIP_OR_FAIL(hipMemcpyAsync(runs.data() + (size_t)i * (size_t)(nlaunch + 1), h->d_run.p,
                                   (size_t)(nlaunch + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIP_OR_FAIL(hipMemcpyAsync(ctl.data() + 2 * i, h->d_ftctl.p, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    }
    if (int rc = group_sync(hs, n)) return rc;
    for (int i = 0; i < n; ++i)
        if (ctl[2 * i + 1]) return fail(GOLHIP_EHIP, "group flip stream: look-back spin bound exceeded on strip %d (board undefined)", i);
    const FlipMergePlan plan = flip_merge_plan(runs.data(), n, nlaunch, cap);
    const int64_t done = plan.done;
    if (done == nlaunch) {
        for (int i = 0; i < n; ++i) hs[i]->alive_turn = hs[i]->turns;
    } else if (done == nlaunch - 1) {
        // only the last turn did not fit: no strip stopped before it, so every
        // strip ran it on valid halos and its source board is the other buffer
        for (int i = 0; i < n; ++i) {
            hs[i]->cur ^= 1;
            hs[i]->turns = t0 + done;
            hs[i]->alive_turn = -1;
        }
    } else {
        // a strip that passed cap by itself stopped there while the others went
        // on beside its stale rows: the boards past turn `done` are void.
        // Restore the batch's first board and step `done` turns (their lists,
        // complete on every strip, are delivered below)
        for (int i = 0; i < n; ++i) {
            golhip *h = hs[i];
            if (int rc = set_dev(h)) return rc;
            HIP_OR_FAIL(hipMemcpyAsync(h->buf[c0[i]] + (int64_t)kHalo * h->Ww, h->backup.p, (size_t)h->local_words() * 4,
                                       hipMemcpyDeviceToDevice, h->stream));
            h->cur = c0[i];
            h->turns = t0;
            h->alive_turn = -1;
        }
        if (done > 0)
            if (int rc = group_step_locked(hs, n, done, 0, ready, false)) return rc;
    }
    // the gather: strip i's segments of the delivered turns to their places in
    // `out`, written by the strip's device where `out` is mapped on it, else
    // into a page-locked list of the batch that the host copies from
    if (plan.total > 0) {
        int mapped_dev = -1;
        char *mapped = (char *)mapped_device_ptr(out, (size_t)plan.total * esz, &mapped_dev);
        bool staged = false;
        for (int i = 0; i < n; ++i) staged |= !(mapped && hs[i]->device == mapped_dev);
        if (staged && g->g_stage_bytes < plan.total * esz) {
            if (g->g_stage) HIP_OR_FAIL(hipHostFree(g->g_stage));
            g->g_stage = nullptr;
            g->g_stage_bytes = 0;
            const size_t want = std::max<size_t>((size_t)plan.total * esz, 1 << 16);
            if (hipError_t e = hipHostMalloc(&g->g_stage, want, hipHostMallocPortable | hipHostMallocMapped); e != hipSuccess) {
                g->g_stage = nullptr;
                return fail(GOLHIP_ENOMEM, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e));
            }
            g->g_stage_bytes = want;
        }
        for (int i = 0; i < n; ++i) {
            golhip *h = hs[i];
            if (runs[(size_t)i * (size_t)(nlaunch + 1) + (size_t)done] == 0) continue;  // nothing of this strip
            if (int rc = set_dev(h)) return rc;
            const bool direct = mapped && h->device == mapped_dev;
            void *dst = mapped;
            if (!direct) HIP_OR_FAIL(hipHostGetDevicePointer(&dst, g->g_stage, 0));
            HIP_OR_FAIL(hipMemcpyAsync(h->d_goff.p, plan.goff.data() + (size_t)i * (size_t)nlaunch,
                                       (size_t)done * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
            golk::FlipGatherArgs a{};
            a.src = reinterpret_cast<const uint32_t *>(h->d_ev.p);
            a.dst = static_cast<uint32_t *>(dst);
            a.run = h->d_run.p;
            a.goff = h->d_goff.p;
            a.nturns = (int)done;
            a.wpe = (unsigned)esz / 4;
            if (int rc = span_begin(h, h->stream)) return rc;
            HIP_OR_FAIL(golk::launch_flip_gather(a, plan.max_seg * a.wpe, h->stream));
            if (int rc = span_end(h, 2)) return rc;
        }
        // second synchronisation
        if (int rc = group_sync(hs, n)) return rc;
        if (staged && !mapped) {
            memcpy(out, g->g_stage, (size_t)plan.total * esz);
        } else if (staged) {
            for (int i = 0; i < n; ++i) {
                if (hs[i]->device == mapped_dev) continue;
                const unsigned long long *r = runs.data() + (size_t)i * (size_t)(nlaunch + 1);
                for (int64_t t = 0; t < done; ++t) {
                    const size_t at = (size_t)plan.goff[(size_t)i * (size_t)nlaunch + (size_t)t] * esz;
                    memcpy((char *)out + at, (char *)g->g_stage + at, (size_t)(r[t + 1] - r[t]) * esz);
                }
            }
        }
    } else if (done < nlaunch) {
        if (int rc = group_sync(hs, n)) return rc;
    }
    for (int i = 0; i < n; ++i) hs[i]->n.flip_entries += (int64_t)runs[(size_t)i * (size_t)(nlaunch + 1) + (size_t)done];
    for (int64_t t = 0; t < done; ++t) counts[t] = plan.counts[(size_t)t];
    if (done > 0) g->group_ft_est = plan.most;
    *done_out = done;
    *total_out = done == 0 ? plan.need : plan.total;
    return GOLHIP_OK;
}

}  // namespace gh

using namespace gh;

extern "C" {

int golhip_flips(golhip_t h, int32_t *xy, uint64_t cap, uint64_t *n) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    if (!h->flips_valid || h->flips_turn != h->turns) {
        if (n) *n = 0;
        return fail(GOLHIP_EINVAL, "no flip list: step with want_flips first");
    }
    // golhip_alive_cells took d_blk and the total for its own list: both boards
    // of the difference are intact, so count and scan again
    if (!h->flips_counted)
        if (int rc = count_flips(h)) return rc;
    return finish_compact(h, h->cur_rows(), h->prev_rows(), xy, cap, n);
}

int golhip_step_flips(golhip_t h, int64_t nturns, int32_t *xy, uint64_t cap, uint64_t *counts, uint64_t *n) {
    if (int rc = check(h)) return rc;
    if (n) *n = 0;
    if (nturns < 0) return fail(GOLHIP_EINVAL, "nturns %lld", (long long)nturns);
    if (nturns > 0 && !counts) return fail(GOLHIP_EINVAL, "counts is null");
    if (cap > 0 && !xy) return fail(GOLHIP_EINVAL, "xy is null");
    std::lock_guard<std::mutex> g(h->mu);
    // The flip kernel's look-back prefixes carry 40-bit offsets: run the batch
    // in chunks whose lists cannot reach 2^40 entries (every cell flipping
    // every turn), each appending after the last.
    const uint64_t cells = std::max<uint64_t>(1, (uint64_t)h->W * (uint64_t)h->rows);
    const int64_t chunk = std::max<int64_t>(1, (int64_t)((1ull << 40) / cells) - 1);
    uint64_t total = 0;
    for (int64_t t = 0; t < nturns || (t == 0 && nturns == 0);) {
        const int64_t m = std::min<int64_t>(chunk, nturns - t);
        const uint64_t got = std::min<uint64_t>(total, cap);
        int64_t done = 0;
        uint64_t part = 0;
        if (int rc = flip_stream_locked(h, m, GOLHIP_FLIPS_XY, xy ? xy + 2 * got : nullptr, cap - got, counts + t, &done,
                                        &part, false))
            return rc;
        total += part;
        t += m;
        if (m == 0) break;
    }
    if (n) *n = total;
    if (total > cap)
        return fail(GOLHIP_ERANGE, "buffer holds %llu cells, %llu needed", (unsigned long long)cap,
                    (unsigned long long)total);
    return GOLHIP_OK;
}

int golhip_flip_stream(golhip_t h, int64_t nturns, int32_t format, void *out, uint64_t cap, uint64_t *counts,
                       int64_t *turns_done, uint64_t *n) {
    if (int rc = check(h)) return rc;
    if (n) *n = 0;
    if (turns_done) *turns_done = 0;
    if (nturns < 0) return fail(GOLHIP_EINVAL, "nturns %lld", (long long)nturns);
    if (format != GOLHIP_FLIPS_XY && format != GOLHIP_FLIPS_INDEX) return fail(GOLHIP_EINVAL, "format %d", format);
    if (nturns > 0 && (!counts || !turns_done || !n)) return fail(GOLHIP_EINVAL, "counts / turns_done / n is null");
    if (cap > 0 && !out) return fail(GOLHIP_EINVAL, "out is null");
    if (format == GOLHIP_FLIPS_INDEX && (uint64_t)h->W * (uint64_t)h->H > (1ull << 32))
        return fail(GOLHIP_EINVAL, "cell indices of a %dx%d board do not fit in 32 bits", h->W, h->H);
    std::lock_guard<std::mutex> g(h->mu);
    if (h->ringed() && h->nranks > 1)
        return fail(GOLHIP_EINVAL, "golhip_flip_stream stops early on one rank alone: use golhip_step_flips in a ring");
    int64_t done = 0;
    uint64_t total = 0;
    if (int rc = flip_stream_locked(h, nturns, format, out, cap, counts, &done, &total, true)) return rc;
    *turns_done = done;
    *n = total;
    if (nturns > 0 && done == 0)
        return fail(GOLHIP_ERANGE, "buffer holds %llu entries, the next turn needs %llu", (unsigned long long)cap,
                    (unsigned long long)total);
    return GOLHIP_OK;
}

int golhip_group_flip_stream(golhip_t *hs, int32_t n, int64_t nturns, int32_t format, void *out, uint64_t cap,
                             uint64_t *counts, int64_t *turns_done, uint64_t *n_entries) {
    if (n_entries) *n_entries = 0;
    if (turns_done) *turns_done = 0;
    if (int rc = group_check(hs, n)) return rc;
    if (n == 1 && hs[0]->torus()) return golhip_flip_stream(hs[0], nturns, format, out, cap, counts, turns_done, n_entries);
    if (nturns < 0) return fail(GOLHIP_EINVAL, "nturns %lld", (long long)nturns);
    if (format != GOLHIP_FLIPS_XY && format != GOLHIP_FLIPS_INDEX) return fail(GOLHIP_EINVAL, "format %d", format);
    if (nturns > 0 && (!counts || !turns_done || !n_entries)) return fail(GOLHIP_EINVAL, "counts / turns_done / n_entries is null");
    if (cap > 0 && !out) return fail(GOLHIP_EINVAL, "out is null");
    if (format == GOLHIP_FLIPS_INDEX && (uint64_t)hs[0]->W * (uint64_t)hs[0]->H > (1ull << 32))
        return fail(GOLHIP_EINVAL, "cell indices of a %dx%d board do not fit in 32 bits", hs[0]->W, hs[0]->H);
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    bool fused = true;  // (but for giant strips)
    for (int i = 0; i < n; ++i) {
        if (hs[i]->turns != hs[0]->turns)
            return fail(GOLHIP_EINVAL, "strip %d is at turn %lld, strip 0 at turn %lld", i, (long long)hs[i]->turns,
                        (long long)hs[0]->turns);
        if (want_il(hs[i]) != want_il(hs[0])) return fail(GOLHIP_EINVAL, "strip %d uses another word layout", i);
        fused &= hs[i]->local_words() < (1ll << 32) - 4096 && hs[i]->fused_flips();
    }
    if (nturns == 0) return GOLHIP_OK;
    // group_exchange's events, made once for the call
    std::vector<hipEvent_t> ready((size_t)n, nullptr);
    int rc = GOLHIP_OK;
    for (int i = 0; i < n; ++i) {
        HIP_RC(hipSetDevice(hs[i]->device));
        HIP_RC(hipEventCreateWithFlags(&ready[i], hipEventDisableTiming));
    }
    int64_t done = 0;
    uint64_t total = 0;
    if (!rc)
        rc = fused ? group_flip_fused(hs, n, nturns, format, out, cap, counts, ready.data(), &done, &total)
                   : group_flip_generic(hs, n, nturns, format, out, cap, counts, ready.data(), &done, &total);
    for (int i = 0; i < n; ++i) {  // (an error may have left work behind the events)
        HIP_RC(hipSetDevice(hs[i]->device));
        if (rc) (void)hipStreamSynchronize(hs[i]->stream);
        if (ready[i]) HIP_RC(hipEventDestroy(ready[i]));
    }
    if (rc) return rc;
    *turns_done = done;
    *n_entries = total;
    if (done == 0)
        return fail(GOLHIP_ERANGE, "buffer holds %llu entries, the next turn needs %llu", (unsigned long long)cap,
                    (unsigned long long)total);
    return GOLHIP_OK;
}

int golhip_alive_cells(golhip_t h, int32_t *xy, uint64_t cap, uint64_t *n) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    const int64_t nw = h->local_words();
    const int64_t nb = golk::compact_blocks(nw);
    if (int rc = h->d_blk.ensure(h, nb)) return rc;
    HIP_OR_FAIL(golk::launch_compact_count(h->cur_rows(), nullptr, nw, h->d_blk.p, h->stream));
    HIP_OR_FAIL(golk::launch_compact_scan(h->d_blk.p, nb, h->d_scalars + 1, h->stream));
    h->flips_counted = false;  // d_blk and the total reused: golhip_flips counts again
    return finish_compact(h, h->cur_rows(), nullptr, xy, cap, n);
}

}  // extern "C"
