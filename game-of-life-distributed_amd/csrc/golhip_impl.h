// golhip_impl.h — what the host units of libgolhip.so share: the handle, the
// error macros and the helpers that cross unit boundaries.  Host side only
// (no kernel): owns the device boards, sequences the step kernels
// (gol_kernels.hip) on one HIP stream, exchanges halo rows with the
// neighbouring strips (RCCL ring or peer copies) and serves the side channels
// (alive count, flip list, alive list, snapshots, frames).
//
// What each entry point replaces in the reference (gol/distributor.go):
//   golhip_create / _load_bytes  world allocation + fill          :66-80
//   golhip_step                  the turn loop                    :93-173
//   golhip_flips                 initializeAliveCells             :212-220
//   golhip_alive_count           len(calculateAliveCells) ticker  :283-302
//   golhip_alive_cells           calculateAliveCells (final)      :180, :420-432
//   golhip_snapshot_bytes        final/s/q raster streams         :186-191, :234-238
//
//   golhip_handle.cpp   handle lifetime, board I/O, counts, hash, perf, trace
//   golhip_plan.cpp     launch planners (decisions on integers + occupancy caches)
//   golhip_step.cpp     step launches, resident guard, RCCL ring, group step
//   golhip_flips.cpp    flip lists and the flip stream (K5, K5r; a group of strips: K5 + gather)
//   golhip_view.cpp     live view of one handle and of a group of strips (K7)
//   golhip_options.cpp  the option table and its consent rules
//   golhip_ckpt.cpp     checkpoints: shadow copy (K8), drain to a file, verified load
//   golhip_image.cpp    PGM images: the same shadow copy, expanded to bytes in page-locked memory (K9), streamed load
//   golhip_stamp.cpp    patterns: an empty board, a rectangle of cells stamped on the torus (K10), pattern files
//   golhip_extract.cpp  saving patterns: any rectangle read back (K12), the alive box (K13), RLE files
//   golhip_rule.cpp     Life-like rules: their spelling, golhip_set_rule; the topology (torus or bounded plane)
//   golhip_pad.cpp      the padded torus and padded strips: widths that are no multiple of 32 on the fast kernels
//
// Everything here but `struct golhip` lives in namespace gh, whose symbols
// are hidden: libgolhip.so exports the C-ABI of include/golhip.h alone.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/golhip.h"
#include "gol_kernels.h"
#include "gol_rule.h"
#include "gol_rule_flip.h"
#include "gol_rule_plane.h"

// Internal linkage across units: nothing in namespace gh is a dynamic symbol.
#define GOLHIP_HIDDEN __attribute__((visibility("hidden")))

namespace gh GOLHIP_HIDDEN {

using golk::kHalo;

// Records the calling thread's last error (golhip_last_error) and returns `code`.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// Turns per launch with an instantiated step kernel (24: one word per lane
// only, as 32; 9: four words per lane only, planned only under a cap of
// exactly 9 (depth_cap); see max_depth_for).
constexpr int kDepths[] = {32, 24, 20, 18, 16, 12, 9, 8, 6, 4, 2, 1};
constexpr int kNumDepths = sizeof(kDepths) / sizeof(kDepths[0]);
// 15 turns: the pair-rule K1w alone, and only in a whole torus' planned tail
// (depth_plan with pair_tail); it has the per-depth caches' last slot.
constexpr int kDepthSlots = kNumDepths + 1;
// trace buffer: 8 totals + (start, end) per (workgroup < 1024, wave < 64)
constexpr int64_t kTraceWords = 8 + 2 * 1024 * 64;

// Grow-only device scratch (contents are not kept): p holds cap elements.
template <typename T>
struct DevScratch {
    T *p = nullptr;
    int64_t cap = 0;
    // Room for n elements, at least `floor` allocated; `zero`: cleared on h's stream when it grows.
    int ensure(golhip *h, int64_t n, bool zero = false, int64_t floor = 1);
    hipError_t release() {
        const hipError_t e = hipFree(p);
        if (e == hipSuccess) {
            p = nullptr;
            cap = 0;
        }
        return e;
    }
};

// What golhip_perf reports and golhip_perf_reset zeroes: the integer counters
// (a step that abandons a resident launch puts them back by copy) ...
struct Counters {
    int64_t step_launches = 0, step_turns = 0;
    int64_t skew_launches = 0, skew_half_launches = 0, pair_launches = 0, pair_turns = 0;
    int64_t persist_launches = 0, persist_turns = 0, lds_launches = 0;
    int64_t halo_exchanges = 0, halo_bytes = 0;
    int64_t flip_launches = 0, flip_entries = 0;
    int64_t flip_resident = 0;  // K5r launches (flip_overlap 2)
    int64_t view_frames = 0;    // frames rendered (K7)
    int64_t pad_launches = 0;   // seam refreshes of the padded torus, one per wide launch
    int64_t rule_launches = 0;  // of step_launches, those on K11 or (a plane) K15
};
// ... and the GOLHIP_FLAG_TIMING sums of the timed spans, by kind (drain_events)
struct Millis {
    double step = 0, persist = 0, flip = 0, halo = 0, view = 0;
};

// What a handle keeps of its checkpoint or image in flight (golhip_ckpt.cpp,
// golhip_image.cpp): whether the shadow has drained to the staging buffers.
// Shared with the job's object, which owns everything else and may be freed first.
struct CkptDrain {
    std::mutex mu;
    std::condition_variable cv;
    bool drained = false;
};

}  // namespace gh

#define HIP_OR_FAIL(expr)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return gh::fail(GOLHIP_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// Accumulating form for loops that must finish their cleanup: sets `rc` once.
#define HIP_RC(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess && rc == GOLHIP_OK)                                                \
            rc = gh::fail(GOLHIP_EHIP, "%s: %s", #expr, hipGetErrorString(e_));                 \
    } while (0)

#define NCCL_OR_FAIL(expr)                                                                              \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess) return gh::fail(GOLHIP_ERCCL, "%s: %s", #expr, ncclGetErrorString(r_)); \
    } while (0)

struct golhip {
    int W = 0, H = 0, Ww = 0;
    int row0 = 0, rows = 0;  // this handle's rows of the torus
    bool strip = false;      // created by golhip_create_strip
    int device = 0;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;

    uint32_t *buf[2] = {nullptr, nullptr};
    int cur = 0;
    int64_t phys_rows = 0;

    int tb_depth = 20;          // per-launch WPL-2 kernels fuse up to 20, the resident kernel 16
    int rows_per_wave = 0;      // 0 = automatic (per depth, from occupancy)
    int cu_count = 0;           // CUs the launches are planned for (option "cu_count": fewer)
    int dev_cu = 0;             // the device's CUs
    int fill_skip = 1;          // option "fill_skip"
    // the Life-like rule (golhip_set_rule): two 9-bit masks, Conway's by default.  A handle with another
    // rule (or, tests, option "rule_kernel") steps on K11 (gol_rule.hip): canonical words, per-launch only
    uint32_t birth = 0x008, survive = 0x00C;
    int rule_kernel = 0;            // option "rule_kernel" (test hook): 1 a Conway handle on K11 too, 2 K11's dynamic policy always
    bool conway() const { return birth == 0x008 && survive == 0x00C; }
    // golhip_set_topology: a bounded plane (every cell outside the board dead at every turn) steps on K15
    // (gol_rule_plane.hip), K11's shape at any width and depth; Conway's rule on its static policy there
    bool plane = false;
    bool rule_path() const { return !conway() || rule_kernel != 0 || plane; }
    // golhip_set_rule_flips: 1 sends the flip streams of a rule_path() handle through K14 (gol_rule_flip.hip),
    // one fused launch a turn; 0 (default) through the step kernel and the three-pass compaction
    int rule_flips = 0;
    bool fused_flips() const { return !plane && (!rule_path() || rule_flips == 1); }  // (K14 has no plane form)
    int last_variant = 1;           // kernel family of the last step launch (golhip_perf kernel_variant)
    int skew = 1;                   // option "skew": skewed band stacks (K1w) for per-launch steps
    int skew_young = 0;             // option "skew_young": band height of waves 4..7, % of waves 0..3's (0: by kernel)
    int skew_hcap = -1;             // option "skew_hcap": rows a stack's bottom band gives up (-1: 3 D / 4)
    int skew_prio = 0;              // option "skew_prio": s_setprio 1 for waves 4..7
    int skew_tx = 0;                // option "skew_tx": tiles per K1w workgroup (0: plan, 1 or 2)
    int skew_half = 0;              // option "skew_half": half-wave tiles (0: when fewer wave-rows, 1: whenever possible, -1: never)
    int lds_bpc[4] = {};               // K1r workgroups per CU by (wpl, 512 / 1024 threads) at lds_bpc_bytes of LDS
    int64_t lds_bpc_bytes[4] = {};
    int lds_bpc_stride[4] = {};
    int skew_bpc[gh::kDepthSlots][12] = {};  // K1w workgroups per CU by (depth, wpl, half, pairs) (0: not queried)
    int skew_pairs = 5;             // option "skew_pairs": the pair rule (8 LUTs a word-turn) at depth 18 (depth_cap)
    bool pair_tail_step = false;    // the step in flight plans its tail from the pair depths 12 / 15 / 16 (pair_tail_on; skew_dims)
    int skew_interior = 1;         // option "skew_interior": K1w's interior main-loop body (gol_skew_span.h; 0: the general body alone)
    unsigned *skew_err = nullptr;      // host-mapped spin-bound flag of the K1w kernels
    unsigned *skew_err_dev = nullptr;
    int lds_band = -1;              // option "lds_band": resident LDS bands K1r (1 on where it fits, 0 off, -1 auto)
    int lds_depth = 0;              // option "lds_depth": turns per K1r super-step (0: plan)
    int lds_xcd = 1;                // option "lds_xcd": consecutive K1r bands on one XCD
    int lds_waves = 0;              // option "lds_waves": K1r waves per workgroup (8 or 16; 0: plan)
    int lds_wg_cu = 1;              // option "lds_wg_cu": K1r bands (workgroups) per CU (1 or 2)
    int lds_stride = 1;             // option "lds_stride": K1r LDS rows at a compile-time stride where instantiated
    int resident_fault = 0;         // option "resident_fault" (tests): K1r band 0 / K1p workgroup 0 never report
                                    // (their neighbours' bounded waits time out: the restore-and-re-run path)
    int lds_age = 0;                // option "lds_age": K1r run rows of a younger wave rank, % of the older's (0: plan)
    int lds_pre = 2;                // option "lds_pre": K1r interior-first turns while the halos travel
                                    // (profiles/r4pre: 8192^2 31.4 -> 33.9 TCUPS at 2; 1: 33.2, 3: 33.1, 4: 32.3)
    gh::DevScratch<uint32_t> lds_edge;  // K1r edge rows (golk::lds_band_edge_words)
    int persistent = -1;        // option "persistent": K1p for long torus runs (1 on, 0 off, -1 auto)
    int wpl_opt = 0;            // option "wpl": words per lane (0 = auto, 1, 2, 4)
    bool no_quads = false;      // the automatic words per lane are 1 or 2 (the wide board of a padded torus)
    int persist_depth = 0;      // option "persist_depth" (0: tb_depth)
    int persist_waves = 0;      // option "persist_waves": waves per workgroup (0: default)
    int paired_bands = 1;       // option "paired_bands": SIMD mates share two bands from both ends (persistent)
    int dummy_rows = 0;         // option "dummy_rows": halo rows taking the kernels' dummy stores (0: all)
    int persist_wg_tx = 0;      // option "persist_wg_tx": tiles across a persistent workgroup (0: plan)
    int persist_half = 1;       // option "persist_half": a D/2-turn remainder runs as the resident kernel's last super-step
    unsigned long long *d_trace = nullptr;  // option "trace": persistent-kernel diagnostics
    unsigned *d_sync = nullptr; // persistent kernel: [0] error, [1..] progress per workgroup
    unsigned *h_err = nullptr;  // pinned copy of the error word
    bool persist_pending = false;
    // resident-launch guard (torus): the board as it was before the step's
    // resident launch, restored and re-run on the per-launch kernels if that
    // launch times out (its workgroups were not all co-resident)
    gh::DevScratch<uint32_t> backup;
    bool guarded = false;
    bool guard_light = false;  // the guarded step is one source-keeping launch: its source is the copy
    // the error word d_sync[0] is sticky over a guarded step: only its first
    // resident launch clears it, so a later launch (steps past resident_max
    // turns, a one-rank ring's rounds) can neither wipe an earlier timeout nor
    // run on a drained board unnoticed (its waits see the word and drain too)
    bool err_clear = true;
    int resident_max = (int)golk::kResidentMaxTurns;  // turns a resident launch takes (test hook "resident_max_turns")
    int64_t persist_fallbacks = 0;
    int64_t persist_timeout_ticks = 100000000ll;  // 1 s at the 100 MHz s_memrealtime clock (option "persist_timeout_us")
    int auto_rpw[gh::kDepthSlots] = {};  // cache per depth index
    bool loaded = false;
    int il = 0;                 // word layout of the board: 0 canonical, 2 interleaved pairs, 4 quads (= wpl)
    std::atomic<int64_t> turns{0};

    // side-channel scratch
    unsigned long long *d_scalars = nullptr;  // [0] alive, [1] compaction total, [2] hash, [3] a ring's count; a checkpoint load: [2] alive, [3] hash
    unsigned long long *h_scalars = nullptr;  // pinned mirror
    int64_t alive_turn = -1;                  // turn whose count sits in d_scalars[0]
    gh::DevScratch<unsigned long long> d_blk;
    gh::DevScratch<int32_t> d_xy;             // (x, y) pairs: two elements a cell
    gh::DevScratch<unsigned long long> d_run;  // flip streams: running list offsets
    // flip stream (K5, golhip_flip_stream / golhip_step_flips)
    gh::DevScratch<unsigned long long> d_ftstatus;  // look-back word per block (zeroed once)
    gh::DevScratch<unsigned> d_ftticket;            // virtual block ids, one counter per turn
    gh::DevScratch<unsigned> d_ftctl;               // [0] stop, [1] look-back spin error
    gh::DevScratch<unsigned char> d_ev;             // entries of a batch
    unsigned flip_epoch = 0;
    int flip_debug = 0;  // option "flip_debug" (measurement only: wrong lists)
    int flip_cp_groups = 4;  // K5r copy-block groups (GOLHIP_TUNING=1 GOLHIP_FLIP_CP_GROUPS=n, 1..8)
    int flip_overlap = 2;  // option "flip_overlap": how lists reach golhip_host_alloc memory (flip_batch)
    gh::DevScratch<unsigned> d_ftdone;  // K5r: kFtShards done counters a turn
    bool ft_ticket = false;       // K5 block order by ticket (set after a co-residency failure)
    uint64_t ft_est = 0;          // most entries of one turn in the last batch (launch sizing)
    int64_t flip_fallbacks = 0;
    // golhip_group_flip_stream (the staging list and the estimate live on the group's first strip)
    gh::DevScratch<unsigned long long> d_goff;  // this strip's segment offsets in `out`, one a turn
    void *g_stage = nullptr;      // page-locked list of a batch whose `out` the strips' devices cannot write
    size_t g_stage_bytes = 0;
    uint64_t group_ft_est = 0;    // most entries of one board turn in the last batch (launch sizing)
    gh::DevScratch<uint8_t> d_stage;    // byte staging for load/snapshot
    gh::DevScratch<uint32_t> d_vcount;  // group view: count rows of the pixel rows that straddle strips
    bool flips_valid = false;
    int64_t flips_turn = -1;
    bool flips_counted = false;   // d_blk and d_scalars[1] still hold the flip list's counts (golhip_alive_cells reuses them)

    // ring
    ncclComm_t comm = nullptr;
    // test hook (golhip_test_ring_init): a ring whose halo exchange runs
    // through a host callback instead of RCCL (two processes on one device)
    golhip_test_transport_fn xport = nullptr;
    void *xport_user = nullptr;
    uint32_t *xport_host = nullptr;  // pinned: send up, send down, recv top, recv bottom
    int64_t xport_cap = 0;           // words per block
    bool ringed() const { return comm || xport; }
    int force_halo = 0;         // option "force_halo": one-rank RCCL ring on a whole board (tests)
    int nranks = 1, rank = 0;
    int ring_rows = 0;          // smallest strip of the ring (every rank plans from it)
    int halo_skip = 0;          // option "halo_skip" (measurement only: no exchange, wrong halos)
    // halo mode: row strips of a multi-rank ring, or (option force_halo) a
    // whole board run as a one-rank RCCL ring
    bool halo_mode() const { return ringed() && (nranks > 1 || force_halo); }

    // measurement
    std::vector<hipEvent_t> ev_pool;
    struct Timed {
        hipEvent_t e0, e1;
        int kind;  // 0 per-launch step, 1 resident step, 2 flip turn (K5), 3 halo exchange, 4 view frame (K7)
    };
    std::vector<Timed> ev_pending;
    hipEvent_t span_e0 = nullptr, span_e1 = nullptr;  // the open timed span (span_begin) ...
    hipStream_t span_stream = nullptr;                // ... and the stream it is recorded on
    gh::Counters n;
    gh::Millis ms;  // (halo: exchange time on the engine stream)

    std::shared_ptr<gh::CkptDrain> ckpt_drain;  // the last golhip_checkpoint_begin / golhip_image_begin on this handle
    // guards ckpt_drain alone (taken inside `mu` where both are held): golhip_drain_wait reads the slot
    // without queueing for `mu`, which a stepping thread takes again and again
    std::mutex drain_mu;

    // the padded torus (golhip_pad.cpp): a whole torus with W % 32 != 0 and no
    // communicator steps as the Wp x H torus `wide` (same device and stream,
    // per-launch kernels only), created at its first such step and destroyed
    // with this handle.  The canonical board here is whole between calls.
    golhip *wide = nullptr;
    int pad_mode = -1;        // golhip_set_pad_step: -1 the measured rule, 0 never, 1 always
    bool pad_nomem = false;   // the wide board could not be allocated: the rule stays on K1g
    // padded strips (golhip_group_step[_ex]): every strip of a group whose
    // width is no multiple of 32 owns the wide strip `wide` (Wp columns, this
    // strip's row0 and rows, its own halo rows); the group decides from strip 0
    int group_pad_mode = -1;        // golhip_group_set_pad_step: -1 the measured rule, 0 never, 1 always
    bool group_pad_nomem = false;   // a wide strip of the group could not be allocated: the rule stays on K1g

    std::mutex mu;

    int64_t local_words() const { return (int64_t)rows * Ww; }
    // (K8's 16-byte loads and stores start at these: kHalo * Ww words are whole 16-byte groups)
    static_assert(golk::kHalo % 4 == 0, "the rows behind the top halo must stay 16-byte aligned");
    uint32_t *cur_rows() const { return buf[cur] + (int64_t)golk::kHalo * Ww; }
    uint32_t *prev_rows() const { return buf[cur ^ 1] + (int64_t)golk::kHalo * Ww; }
    bool torus() const { return nranks == 1 && rows == H; }
};

namespace gh GOLHIP_HIDDEN {

template <typename T>
int DevScratch<T>::ensure(golhip *h, int64_t n, bool zero, int64_t floor) {
    if (cap >= n) return GOLHIP_OK;
    if (p) HIP_OR_FAIL(hipFree(p));
    p = nullptr;
    cap = 0;
    const int64_t want = std::max(n, floor);
    if (hipError_t e = hipMalloc((void **)&p, (size_t)want * sizeof(T)); e != hipSuccess) {
        p = nullptr;
        return fail(GOLHIP_EHIP, "hipMalloc(%lld x %zu bytes): %s", (long long)want, sizeof(T), hipGetErrorString(e));
    }
    if (zero) HIP_OR_FAIL(hipMemsetAsync(p, 0, (size_t)want * sizeof(T), h->stream));
    cap = want;
    return GOLHIP_OK;
}

// ---- golhip_handle.cpp ----------------------------------------------------
int check(golhip_t h);    // a non-null handle
int set_dev(golhip_t h);  // hipSetDevice(h->device)
// Device address of [p, p + bytes) if it lies inside one golhip_host_alloc buffer.
void *mapped_device_ptr(const void *p, size_t bytes, int *device = nullptr);
// A timed span of work on stream `st`: two events around it, their time added
// to the sum of `kind` (golhip::Timed) at the next drain.  Nothing is
// recorded without GOLHIP_FLAG_TIMING.  One span at a time per handle.
// drain: the pending spans are summed here once 4096 have gathered (this
// synchronises on their events; per-launch steps and view frames, whose count
// a caller's golhip_perf calls do not bound).
int span_begin(golhip_t h, hipStream_t st);
int span_end(golhip_t h, int kind, bool drain = false);
int drain_events(golhip_t h);
int take_skew_err(golhip_t h);
int sync_stream(golhip_t h);  // synchronise, then take_skew_err and the resident launch's flag
int set_layout(golhip_t h, int il);
int loaded_canonical(golhip_t h);  // after canonical words were written into the current buffer

// ---- golhip_plan.cpp --------------------------------------------------------
struct DepthRun {
    int d;
    int64_t n;
};
struct HaloRun {
    int d, k;
};
int largest_depth(int64_t want);
DepthRun depth_plan(int cap, int64_t left, bool pair_tail = false);
bool pair_tail_on(golhip_t h);
int sched_rows(golhip_t h);
int persist_nw_for(golhip_t h, int depth, int wpl);
bool persist_on(golhip_t h);
int wpl_for(golhip_t h);
int want_il(golhip_t h);
int depth_cap(golhip_t h, bool halo);
int next_depth(golhip_t h, int64_t remaining, bool halo);
bool tb_paired(golhip_t h);
int rows_per_wave_for(golhip_t h, int depth);
void halo_plan(int strip_rows, int nranks, int rank, int depth, int Ww, golhip_halo_plan_t *p);
bool skew_dims(golhip_t h, int depth, int wpl, int L, golk::SkewArgs *sk);
bool skew_plan(golhip_t h, int depth, int wpl, const golk::StepArgs &a, golk::SkewArgs *sk);
int halo_launches(int rows, int depth, int64_t run);
HaloRun halo_next(int cap, int rows, bool resident, int64_t left);
bool lds_fits(golhip_t h, int wpl, golk::LdsBandArgs *out = nullptr);
int persist_depth_for(golhip_t h, int wpl);

// ---- golhip_step.cpp --------------------------------------------------------
golk::StepArgs step_args(golhip_t h, unsigned long long *alive, bool halo);
int exchange_rccl(golhip_t h, int depth, hipStream_t st);
int launch_depth(golhip_t h, int depth, bool count, bool halo);
int step_checked_locked(golhip_t h, int64_t nturns, int32_t want_flips);
int group_check(golhip_t *hs, int32_t n, bool need_board = true);  // need_board: every strip loaded
// pad false: no padded strips (the flip stream's re-run of a stopped batch).
int group_step_locked(golhip_t *hs, int32_t n, int64_t nturns, int32_t want_flips, hipEvent_t *keep = nullptr,
                      bool pad = true);
// The rounds of a group step: `turns` turns of the strips ss (a group's own
// strips, or their wide strips with `owners` set: then a seam refresh of the
// rows it reads goes before every launch, pad_seam), deep-halo exchanges
// through `ready`.  count_last: the last launch leaves every strip's count.
int group_rounds(golhip_t *ss, golhip_t *owners, int32_t n, int64_t turns, bool count_last, hipEvent_t *ready);
// Halo rows of every strip from its ring neighbours' current boards, x rows
// each way, by peer copies ordered through the n events `ready`.  relaunch:
// several launches may follow before the next exchange, so every stream also
// waits for its neighbours' copies (false: exactly one single-turn launch a
// strip follows, as in the group flip stream).
int group_exchange(golhip_t *hs, int32_t n, int x, hipEvent_t *ready, bool relaunch = true);

// ---- golhip_flips.cpp -------------------------------------------------------
int start_flips(golhip_t h);

// ---- golhip_ckpt.cpp (the drain job's parts, shared with golhip_image.cpp) ----
// One strip's share of a job that drains a shadow copy of the board: its
// shadow and the events around its kernel (K8, launch_ckpt).
struct ShadowPart {
    int device = 0;
    int64_t row0 = 0, rows = 0;
    uint32_t *shadow = nullptr;
    unsigned long long *d_sums = nullptr;  // [0] alive, [1] digest
    hipEvent_t k0 = nullptr, k1 = nullptr; // around the kernel on the handle's stream
    hipStream_t side = nullptr;            // the device's side stream (owned by the first part on it)
    bool own_side = false;
};
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0);
// opts->chunk_rows, or (0) the rows of row_bytes bytes that fit 16 MiB, at least one (golimg::chunk_rows_for)
int chunk_rows_for(const golhip_ckpt_opts_t *opts, int64_t row_bytes, int *out);
bool write_all(int fd, const void *p, size_t bytes, uint64_t off);  // pwrite until done
bool read_all(int fd, void *p, size_t bytes, uint64_t off);         // pread until done (false: short file)
// The tail of a drain job's writer: with `ok` (nothing failed so far) the
// header at offset 0, fsync; close; rename of tmp over path; a tmp that was
// opened and not renamed is unlinked.  False with *what naming the first call
// that failed here (errno is that call's), or null where `ok` came in false.
bool file_commit(int fd, const std::string &tmp, const std::string &path, const void *head, size_t head_bytes, bool ok,
                 const char **what);
void drain_set(CkptDrain &d);
// Waits until the earlier job of each handle has left the device (it neither joins nor frees it).
void drain_wait_earlier(golhip_t *hs, int32_t n);
// Shadow, sums, events and side stream of every strip (`what` names the job in messages).
int shadow_alloc(golhip_t *hs, int32_t n, const char *what, std::vector<ShadowPart> &parts, int *max_rows);
// Under every strip's mutex: one turn for all (*turn), K8 on each handle's
// stream, the side stream behind it, `drain` left with the handle.
int shadow_enqueue(golhip_t *hs, int32_t n, std::vector<ShadowPart> &parts, const std::shared_ptr<CkptDrain> &drain,
                   int64_t *turn);
void shadow_kernels_wait(std::vector<ShadowPart> &parts);  // the kernels have run to their end
double shadow_stall_ms(std::vector<ShadowPart> &parts);    // device time of the kernels, summed
// Waits for the kernels and the side streams, then frees what shadow_alloc made.
int shadow_free(std::vector<ShadowPart> &parts);

// ---- golhip_pad.cpp ---------------------------------------------------------
bool pad_applies(golhip_t h);                // a whole torus, W % 32 != 0, no communicator
bool pad_wanted(golhip_t h, int64_t nturns);  // this step of nturns turns takes the padded path
// nturns >= 1 turns of h on its wide board: pad, seam + launch for each launch
// of the wide board's plan, unpad with the count.  *ran false (rc 0): the wide
// board could not be had and the rule falls back to K1g.
int pad_step(golhip_t h, int64_t nturns, bool *ran);
int pad_destroy(golhip_t h);                 // the wide board, if any (golhip_destroy)
// Padded strips: whether this group_step call of nturns turns pads (every strip or none) ...
bool pad_group_wanted(golhip_t *hs, int32_t n, int64_t nturns);
// ... and the call itself: pad, group_rounds over the wide strips, unpad with
// every strip's own count.  *ran false (rc 0): a wide strip could not be had
// and the rule falls back to K1g for the group's life.
int pad_group_step(golhip_t *hs, int32_t n, int64_t nturns, hipEvent_t *ready, bool *ran);
// The ghosts of the wide rows [lo, hi) of h's wide strip (relative to the
// strip's first row; halo rows included), rewritten from their real columns.
int pad_seam(golhip_t h, int lo, int hi);

// ---- golhip_options.cpp -----------------------------------------------------
bool tuning_env();      // GOLHIP_TUNING=1 (or GOLHIP_MEASUREMENT=1)
bool test_hooks_env();  // GOLHIP_TEST_HOOKS=1

}  // namespace gh
