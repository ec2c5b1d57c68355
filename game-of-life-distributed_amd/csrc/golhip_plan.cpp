// golhip_plan.cpp — the launch planners: which kernel, how many turns a
// launch, words per lane, band and stack shapes.  Decisions on plain integers
// plus occupancy queries cached in the handle; nothing is launched here.
#include "golhip_impl.h"
#include "gol_skew_span.h"
#include <climits>
#include <functional>

namespace gh GOLHIP_HIDDEN {

// Depth 9 (quads only) is never a "largest depth": the resident kernels and
// the other word widths have no 9.
int largest_depth(int64_t want) {
    for (int d : kDepths)
        if (d <= want && d != 9 && d != 18) return d;
    return 1;
}
// Depths a plan capped at exactly them alone takes: 9 (quads) and 18 (the
// pair-rule K1w, option "skew_pairs"); depth_cap.
static bool special_depth(int d) { return d == 9 || d == 18; }

// The next run of launches for `left` turns of at most `cap` turns each:
// depth d and how many launches of d come next.  The schedule has the fewest
// launches and, among those, the largest smallest launch, in descending
// order: 100 turns at cap 16 run as 4 x 16 + 3 x 12, not 6 x 16 + 4 (a
// 4-turn launch costs about as much as a 16-turn one on a large board:
// 65536^2 x 100 turns ran at 108 vs 122 TCUPS kernel-only).  Far from the
// end the run is `cap` turns; the last 12-13 caps are planned exactly
// (262144^2 x 100 turns at cap 9: 4 x 9 + 8 x 8, not 8 x 9 + 2 x 8 + 2 x 6,
// which a plan of only the last 3-4 caps found).
//
// pair_tail (a whole torus on the pair rule's full-width tiles, pair_tail_on):
// the planned tail may also take the pair kernel's own remainder depths (12,
// 15, 16), and the schedule is the one of least estimated cost, a launch of d
// turns costing (d + r) x slots(d): r turns' worth of ramps, 12 issue slots a
// word-turn on the pair rule and 13 on the 9-LUT stages.
// The fewest-launches schedule stays wherever the estimate finds nothing
// cheaper, its 12s and 16s on the pair kernel: 1,000 turns run 52 x 18 + 4 x 16
// as before, 999 run 53 x 18 + 3 x 15 where they ran 55 x 18 + 8 + 1.
static constexpr int kPairTailDepths[] = {18, 16, 15, 12, 8, 6, 4, 2, 1};
// r in tenths of a turn, fitted to the 18-turn pair launch and the 16-turn
// 9-LUT launch of profiles/pair_tail/step0_kernel_trace.json
static constexpr int kRampTenths = 281;
static int64_t launch_cost(int d, bool pair_kernel) { return (int64_t)(10 * d + kRampTenths) * (pair_kernel ? 12 : 13); }
static bool pair_tail_depth(int d) { return d == 18 || golk::skew_pair_tail_depth(d); }

static DepthRun first_run(std::vector<int> &seq, int M, int64_t head) {
    std::sort(seq.begin(), seq.end(), std::greater<int>());
    const int d = head > 0 ? M : seq[0];
    int64_t n = head;
    for (int x : seq) n += (x == d);
    return {d, n};
}

DepthRun depth_plan(int cap, int64_t left, bool pair_tail) {
    const int M = special_depth(cap) ? cap : largest_depth(std::max(1, cap));  // 9: quads, 18: pairs (depth_cap)
    if (left <= 0) return {M, 0};
    const int64_t head = std::max<int64_t>(0, left / M - 12);  // launches of M before the planned tail
    const int t = (int)(left - head * M);                      // < 13 M <= 416
    std::vector<int> cheap;
    int64_t cheap_cost = -1;
    if (pair_tail && M == 18) {
        // least cost; then fewest launches, then the largest smallest launch
        std::vector<int64_t> cost(t + 1, INT64_MAX);
        std::vector<int> nl(t + 1, 0), mn(t + 1, INT_MAX), pick(t + 1, 0);
        cost[0] = 0;
        for (int v = 1; v <= t; ++v)
            for (int d : kPairTailDepths) {
                if (d > v) continue;
                const int64_t c = cost[v - d] + launch_cost(d, pair_tail_depth(d));
                const int n = nl[v - d] + 1, m = std::min(mn[v - d], d);
                if (c < cost[v] || (c == cost[v] && (n < nl[v] || (n == nl[v] && m > mn[v])))) {
                    cost[v] = c;
                    nl[v] = n;
                    mn[v] = m;
                    pick[v] = d;
                }
            }
        for (int v = t; v > 0; v -= pick[v]) cheap.push_back(pick[v]);
        cheap_cost = cost[t];
    }
    // best[v] = (launches, -smallest launch) for v turns; pick[v] = first depth
    std::vector<int> nl(t + 1, INT_MAX), mn(t + 1, 0), pick(t + 1, 0);
    nl[0] = 0;
    mn[0] = INT_MAX;
    for (int v = 1; v <= t; ++v)
        for (int d : kDepths) {  // descending: ties keep the larger depth
            if (d > M || d > v || nl[v - d] == INT_MAX || (special_depth(d) && M != d)) continue;
            const int n = nl[v - d] + 1, m = std::min(mn[v - d], d);
            if (n < nl[v] || (n == nl[v] && m > mn[v])) {
                nl[v] = n;
                mn[v] = m;
                pick[v] = d;
            }
        }
    std::vector<int> seq;
    for (int v = t; v > 0; v -= pick[v]) seq.push_back(pick[v]);
    if (cheap_cost >= 0) {
        // ties keep that schedule (its 12s and 16s run on the pair kernel here too)
        int64_t c = 0;
        for (int x : seq) c += launch_cost(x, pair_tail_depth(x));
        if (cheap_cost < c) return first_run(cheap, M, head);
    }
    return first_run(seq, M, head);
}

// Rows the launch schedule (depth, exchange depth, words per lane) is derived
// from: in a multi-rank ring every rank must pick the same values, so they
// all use the ring's smallest strip.
int sched_rows(golhip_t h) { return (h->ringed() && h->nranks > 1 && h->ring_rows > 0) ? h->ring_rows : h->rows; }

// Relative rate of a (words per lane, waves per workgroup) choice for the
// persistent torus kernel: stored fraction of the computed tile words x band
// efficiency S / (S + 1.75 D) (pipeline fill, see stream_band) x occupancy /
// VALU slots per word-turn (wpl 1: 9 LUT + 2 half-rate shifts + 2 half-rate
// DPP = 17 slots; wpl 2 interleaved: 9 + 1 + 1 half-rate = 13).  Fitted to
// the round-1c sweeps (profiles/r1c): 16384^2 -> wpl 1 with 8 waves,
// 65536^2 -> wpl 2.
// VALU slots per word-turn: 9 LUTs + 2 half-rate DPP moves and 2 half-rate
// funnel shifts per WPL words (interleaved layouts for WPL 2 and 4).
static double slots_per_word(int wpl) { return 9.0 + 8.0 / wpl; }

static double plan_rate(golhip_t h, int wpl, int nw, int depth) {
    const int tiles = golk::tb_tiles(h->Ww, wpl);
    const double util = (double)h->Ww / (tiles * 62.0 * wpl);
    const double S = (double)sched_rows(h) * tiles / std::max(1.0, (double)h->cu_count * nw);
    const double occ = nw >= 16 ? 1.0 : 0.95;
    return util * S / (S + 1.75 * depth) * occ / slots_per_word(wpl);
}

static int default_depth(golhip_t h, int wpl) { return largest_depth(std::min(h->tb_depth, golk::persist_max_depth(wpl))); }

// Waves per workgroup of the persistent kernel: the option, or the better of
// 16 (4 per SIMD: hides VALU latency) and 8 (taller bands: less fill).
int persist_nw_for(golhip_t h, int depth, int wpl) {
    if (h->persist_waves > 0) return h->persist_waves;
    const int def = golk::persist_waves_for(depth, wpl);
    if (def == 16 && plan_rate(h, wpl, 8, depth) > plan_rate(h, wpl, 16, depth) &&
        golk::persist_blocks_per_cu(depth, wpl, 8) >= 1)  // (depth, wpl, 8) instantiated
        return 8;
    return def;
}

// The resident kernel wins on boards whose two buffers sit in the 256 MB
// MALL (16384^2: 61 vs 58 TCUPS); on larger boards the per-launch kernel is
// as fast or faster and far steadier from box to box (65536^2: 114-116 vs
// 96-120 TCUPS over six boxes, 262144^2: 126 vs 105, profiles/r1f), so
// "auto" keeps K1p for buffers of at most 64 MiB (sched_rows: every rank of
// a ring decides alike, as the choice also fixes the word layout).  A row
// strip runs K1p between two deep-halo exchanges (golhip_step).
static constexpr int64_t kPersistAutoMaxBytes = 64ll << 20;
static int wpl_per_launch(golhip_t h);
static bool skew_fills(golhip_t h);
bool persist_on(golhip_t h) {
    if (h->rule_path()) return false;  // K11 has no resident form
    // a multi-rank ring never runs the resident kernel (try_persist_halo):
    // plan words per lane and halos for the per-launch kernels that do run
    if (h->ringed() && h->nranks > 1) return false;
    if (h->persistent >= 0) return h->persistent != 0;
    // round 3: K1w per launch wherever its stacks fill the CUs (16384^2: 82
    // vs 62 TCUPS); smaller boards keep the resident kernel (8192^2: 27.9
    // vs 21.7 for K1w and 12.8 for the per-launch K1, profiles/r3i)
    if (h->skew && skew_fills(h)) return false;
    return (int64_t)sched_rows(h) * h->Ww * 4 <= kPersistAutoMaxBytes;
}

// Words per lane of the step kernels: 2 (interleaved pair layout) cuts the
// shift work per word but quantises tiles at 124 words and halves the band
// height; the option, or whichever plan_rate prefers.
int wpl_for(golhip_t h) {
    if (h->W % 64 != 0 || h->rule_path()) return 1;  // (K11: canonical words, one a lane)
    if (h->wpl_opt == 1 || h->wpl_opt == 2) return h->wpl_opt;
    if (h->wpl_opt == 4) return h->W % 128 == 0 ? 4 : 2;
    if ((!h->torus() && !h->ringed()) || !persist_on(h)) return wpl_per_launch(h);
    if (lds_fits(h, 2)) return 2;  // K1r: pairs (11 slots a word-turn against 15)
    auto best = [&](int wpl) {
        const int d = default_depth(h, wpl);
        const int def = golk::persist_waves_for(d, wpl);
        return std::max(plan_rate(h, wpl, def, d), def == 16 ? plan_rate(h, wpl, 8, d) : 0.0);
    };
    // The model charges WPL 2's halved bands too much fill: at 16384^2 it
    // prefers WPL 1 by 4 %, but WPL 2 (8 waves) measured 61.7 vs 59.0 TCUPS
    // on the same box (profiles/r2p/persist_wpl_16384.txt), so WPL 2 wins
    // unless the model puts it more than 5 % behind.
    return best(2) >= 0.95 * best(1) ? 2 : 1;
}

// Words per lane of the per-launch kernels (the option, else the rate model).
static int wpl_per_launch(golhip_t h) {
    if (h->W % 64 != 0) return 1;
    if (h->wpl_opt == 1 || h->wpl_opt == 2) return h->wpl_opt;
    if (h->wpl_opt == 4) return h->W % 128 == 0 ? 4 : 2;
    {
        // per-launch kernels (group strips, large boards): the hardware refills freed wave
        // slots, so band height matters less; stored fraction / slots per word
        // (16384-wide strips: 55.6 vs 51.2 TCUPS for wpl 2 vs 1, profiles/r1e)
        // Four words per lane (interleaved quads, 11 slots) run at most 8
        // turns a launch (226 VGPRs); 8- vs 16-turn launches cost ~10 % per
        // turn (fill, twice the HBM passes).  Measured, four vs two words per
        // lane: 131072^2 127.6 vs 120.1 TCUPS, 262144^2 130.8 vs 122.4,
        // 262144 x 32768 (an 8-GPU strip) 124.6 vs 118.5, but 65536^2 107.1
        // vs 115.1 (9 tiles of 248 words for 2048), profiles/r1k; the model
        // gives 65536^2 +0.5 %, hence the 3 % margin.
        auto rate = [&](int wpl) {
            const double deep = (wpl == 4 && h->tb_depth > golk::max_depth_for(4)) ? 0.9 : 1.0;
            return (double)h->Ww / (golk::tb_tiles(h->Ww, wpl) * 62.0 * wpl) / slots_per_word(wpl) * deep;
        };
        const int two = rate(2) >= rate(1) ? 2 : 1;
        // (the wide board of a padded torus pays a seam refresh a launch and
        // takes quads, at most 9 turns a launch, only when asked to: golhip_pad.cpp)
        return (!h->no_quads && h->W % 128 == 0 && rate(4) > 1.03 * rate(two)) ? 4 : two;
    }
}

int want_il(golhip_t h) { return wpl_for(h) >= 2 ? wpl_for(h) : 0; }

// Most turns one launch may fuse.  In halo mode the `depth` halo rows must
// all come from one neighbour strip, so depth <= strip rows.
int depth_cap(golhip_t h, bool halo) {
    if (h->W % 32 != 0 && !h->plane) return 1;  // generic kernel: one turn per launch (a plane has no row seam: K15)
    if (h->rule_path()) {
        // K11's depths (gol_rule.h): every depth depth_plan returns under 16; a
        // cap of exactly 9 would name the quads' own depth
        int cap = std::min(h->tb_depth, golk::kRuleMaxDepth);
        if (halo) cap = std::min(cap, sched_rows(h));
        return cap == 9 ? 8 : cap;
    }
    // a strip between exchanges runs the resident kernel (its depths) when on
    const int wpl = wpl_for(h);
    int cap = std::min(h->tb_depth, (halo && persist_on(h)) ? golk::persist_max_depth(wpl) : golk::max_depth_for(wpl));
    if (halo) cap = std::min(cap, sched_rows(h));
    // the pair rule (option "skew_pairs", round 6): K1w at 18 turns a launch
    // (the pair state's VGPR bound at two words per lane): whole tori, and
    // ring strips (every rank decides from the ring's smallest strip; the
    // extended rows of a strip's launches only make the stacks easier to
    // plan).  Bit 1: plans on full-width tiles; bit 4: half-wave tile plans
    // too (16384^2 87.9 vs 86.4 TCUPS at 16 on the 9-LUT stages, profiles/r7c)
    bool pair = false;
    if ((h->skew_pairs & 1) && wpl == 2 && cap >= 18) {
        golk::SkewArgs sk{};
        if (skew_dims(h, 18, 2, halo ? sched_rows(h) : h->rows, &sk) && (!sk.half || (h->skew_pairs & 4))) {
            cap = 18;
            pair = true;
        }
    }
    // other whole tori whose K1w plan takes half-wave tiles (bands of ~2D
    // rows, the launch mostly ramps) fuse 16 turns: 16384^2
    // 86.3-86.5 vs 85.5-85.7 TCUPS at 20 (profiles/r5v; 82.1 vs 81.2 in r4y)
    if (!pair && !halo && wpl == 2 && cap > 16) {
        golk::SkewArgs sk{};
        if (skew_dims(h, 20, 2, h->rows, &sk) && sk.half) cap = 16;
    }
    if (cap == 9 && (wpl != 4 || (halo && persist_on(h)))) cap = 8;  // only per-launch quads have 9
    // only the pair rule has 18 (depth_plan would take a cap of exactly 18 as
    // its own): a tb_depth of 18, or a schedule planned from 18 rows, at one
    // word per lane has no kernel at all
    if (cap == 18 && !pair) cap = 16;
    // quads (bit 2): 8 turns a launch on the pair rule instead of 9 on the 9-LUT stages
    if ((h->skew_pairs & 2) && wpl == 4 && cap >= 8) {
        golk::SkewArgs sk{};
        if (skew_dims(h, 8, 4, halo ? sched_rows(h) : h->rows, &sk) && !sk.half) cap = 8;
    }
    return cap;
}

// How many turns the next launch fuses (depth_plan).
int next_depth(golhip_t h, int64_t remaining, bool halo) { return depth_plan(depth_cap(h, halo), remaining).d; }

static int depth_index(int d) {
    for (int i = 0; i < kNumDepths; ++i)
        if (kDepths[i] == d) return i;
    return d == 15 ? kNumDepths : kNumDepths - 1;  // (15: the pair rule's remainder depth, kDepthSlots)
}

// Per-launch kernel with paired bands (gol_tb_pair_kernel; needs the fill skip).
bool tb_paired(golhip_t h) { return h->paired_bands && h->fill_skip; }

// Rows per wave for a launch of `depth` turns: the user's value, or the
// automatic choice (wave slots = CUs x resident waves per CU).
int rows_per_wave_for(golhip_t h, int depth) {
    if (h->rows_per_wave > 0) return h->rows_per_wave;
    int &c = h->auto_rpw[depth_index(depth)];
    if (c == 0 && h->rule_path()) {
        const int slots =
            h->cu_count * (h->plane ? golk::plane_wave_slots_per_cu(depth, h->birth, h->survive, h->rule_kernel == 2)
                                    : golk::rule_wave_slots_per_cu(depth, h->W, h->birth, h->survive, h->rule_kernel == 2));
        c = golk::auto_rows_per_wave(h->Ww, h->rows, depth, std::max(slots, 1), false, 1, false);
    }
    if (c == 0) {
        const int wpl = wpl_for(h);
        const int slots = h->cu_count * golk::tb_wave_slots_per_cu(depth, wpl, tb_paired(h));
        c = golk::auto_rows_per_wave(h->Ww, h->rows, depth, std::max(slots, 1), h->fill_skip, wpl, tb_paired(h));
    }
    return c;
}

// Halo plan shared by the RCCL ring and the in-process group.
void halo_plan(int strip_rows, int nranks, int rank, int depth, int Ww, golhip_halo_plan_t *p) {
    p->prev_rank = (rank - 1 + nranks) % nranks;
    p->next_rank = (rank + 1) % nranks;
    p->rows = depth;
    p->send_up_row = kHalo;                               // my first `depth` rows -> prev's bottom halo
    p->recv_bottom_row = kHalo + strip_rows;              // <- next's first rows
    p->send_down_row = kHalo + strip_rows - depth;        // my last rows -> next's top halo
    p->recv_top_row = kHalo - depth;                      // <- prev's last rows
    p->bytes = (int64_t)depth * Ww * 4;
}

// Skewed band stacks (K1w, option "skew"): any per-launch step (whole torus
// or a strip's extended rows) whose depth and words per lane have an
// instance.  One workgroup of 8 waves per stack, sized to fill every CU once:
// as many stacks per tile column as the CUs allow, with bands of at least
// D + 3 rows (any height is exact; shorter bands would mostly wait for the
// band below's exports) and the stack's bottom band `hcap` rows shorter (it
// computes its drain in full).  tx = 2 (stacks of 4
// bands, two tiles a workgroup) when the tile count fits the CUs better.
static int skew_bpc(golhip_t h, int depth, int wpl, bool half, bool pr) {
    int &c = h->skew_bpc[depth_index(depth)][(wpl == 4 ? 2 : wpl - 1) + (half ? 3 : 0) + (pr ? 6 : 0)];
    if (c == 0) {
        const int b = golk::skew_blocks_per_cu(depth, wpl, half, pr);
        c = b > 0 ? b : -1;
    }
    return c;
}

// The stack plan of a K1w launch over L rows: tiles, workgroup shape, stacks
// and tile kind (no side effects); false if K1w does not apply.
static bool skew_dims_for(golhip_t h, int depth, int wpl, int L, bool tail, golk::SkewArgs *sk) {
    // the pair rule: 18 turns at two words per lane (option "skew_pairs" bit
    // 1; no other K1w runs 18: a strip whose group plans 18 without the bit
    // takes the per-launch kernel), 8 at four (bit 2); `tail`: 12, 15 and 16 at
    // two, only in a step whose plan drew on them (depth_plan's pair_tail)
    const bool pr = (depth == 18 && (h->skew_pairs & 1)) || (wpl == 4 && depth == 8 && (h->skew_pairs & 2)) ||
                    (tail && wpl == 2 && golk::skew_pair_tail_depth(depth) && golk::skew_supported(depth, 2, false, true));
    if (!h->skew || h->W % 32 != 0 || !golk::skew_supported(depth, wpl, false, pr)) return false;
    const int hcap = h->skew_hcap >= 0 ? h->skew_hcap : 3 * depth / 4;
    const int smin = depth + 3;
    // half-wave tiles (30 stored lanes a tile, two tiles a wave, the upper one
    // L / 2 rows down): when they need fewer wave-rows than 62-lane tiles
    // (16384^2: 4.5 vs 5 waves a row), or when forced; L must be even
    const bool half_ok = h->skew_half >= 0 && L % 2 == 0 && golk::skew_supported(depth, wpl, true, pr);
    int best_tx = 0, best_nst = 0, best_half = 0, best_tiles = 0;
    double best = 1e300;
    for (int half = 0; half <= (half_ok ? 1 : 0); ++half) {
        if (!half && half_ok && h->skew_half > 0) continue;  // forced
        const int bpc = skew_bpc(h, depth, wpl, half, pr);
        if (bpc < 1) continue;
        const int tiles = half ? (h->Ww + golk::kHalfTileValid * wpl - 1) / (golk::kHalfTileValid * wpl)
                               : golk::tb_tiles(h->Ww, wpl);
        const int Lh = half ? L / 2 : L;
        for (int tx = 1; tx <= 2; ++tx) {
            if (h->skew_tx && tx != h->skew_tx) continue;
            const int sy = 8 / tx, tcols = (tiles + tx - 1) / tx;
            // stacks of Lh / nst + hcap rows whose bands average at least smin + hcap
            // rows (the bottom band gives up hcap of them)
            const int nst = std::min(h->cu_count * bpc / tcols,
                                     Lh / (sy * (smin + hcap) - hcap));
            if (nst < 1) continue;
            // "skew" 1 (default): only when the stacks fill at least 3/4 of the CUs'
            // workgroup slots (smaller tori run the resident kernel, persist_on);
            // 2: whenever a plan exists (tests)
            if (h->skew == 1 && (int64_t)nst * tcols * 4 < (int64_t)h->cu_count * bpc * 3) continue;
            // a wave's buffer-store range (its band, plus L / 2 rows for half tiles) must stay < 2 GiB
            if (((double)Lh / nst + hcap + (half ? Lh : 0)) * h->Ww * 4 >= 2147483648.0) continue;
            // input rows a wave streams; half tiles pay ~2 % for per-lane row addressing
            const double per_wave = ((double)Lh / nst + hcap) / sy * (half ? 1.02 : 1.0);
            if (per_wave < best * 0.999) {
                best = per_wave;
                best_tx = tx;
                best_nst = nst;
                best_half = half;
                best_tiles = tiles;
            }
        }
    }
    if (!best_tx) return false;
    sk->tiles_x = best_tiles;
    sk->pairs = pr ? 1 : 0;
    sk->interior = h->skew_interior && golk::skew_interior_instance(depth, wpl, best_half != 0, pr);
    sk->tx = best_tx;
    sk->nst = best_nst;
    sk->half = best_half;
    sk->hcap = hcap;
    return true;
}

bool skew_dims(golhip_t h, int depth, int wpl, int L, golk::SkewArgs *sk) {
    return skew_dims_for(h, depth, wpl, L, h->pair_tail_step, sk);
}

// Whether this handle's own steps plan their tail from the pair depths
// (depth_plan's pair_tail): a whole torus stepped by itself whose K1w plan
// runs the pair rule on full-width tiles (depth_cap's 18), with a stack plan
// for every remainder instance too.  Rings, groups of strips, the wide board
// of a padded torus, half-tile plans, quads and the Life-like rules are not.
bool pair_tail_on(golhip_t h) {
    if (!h->torus() || h->halo_mode() || h->rule_path() || !(h->skew_pairs & 1)) return false;
    if (depth_cap(h, false) != 18) return false;  // (18 only ever with the pair rule on)
    for (int d : {18, 16, 15, 12}) {
        golk::SkewArgs sk{};
        if (!golk::skew_supported(d, 2, false, true) || !skew_dims_for(h, d, 2, h->rows, true, &sk) || sk.half ||
            !sk.pairs)
            return false;
    }
    return true;
}

// Whether K1w would run this handle's whole-launch steps (its stacks fill
// the CUs at the per-launch words per lane and depth); persist_on keeps the
// resident kernel for the tori where it would not.
static bool skew_fills(golhip_t h) {
    if (!h->skew || h->W % 32 != 0) return false;
    const int wpl = wpl_per_launch(h);
    int cap = std::min(h->tb_depth, golk::max_depth_for(wpl));
    if (cap == 9 && wpl != 4) cap = 8;
    const int depth = cap == 9 ? 9 : largest_depth(cap);
    golk::SkewArgs sk{};
    return skew_dims(h, depth, wpl, sched_rows(h), &sk);
}

bool skew_plan(golhip_t h, int depth, int wpl, const golk::StepArgs &a, golk::SkewArgs *sk) {
    if (!skew_dims(h, depth, wpl, a.rows_out, sk)) return false;
    if (!h->skew_err) {
        void *p = nullptr, *d = nullptr;
        if (hipHostMalloc(&p, sizeof(unsigned), hipHostMallocMapped) != hipSuccess) return false;
        if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) {
            (void)hipHostFree(p);
            return false;
        }
        h->skew_err = static_cast<unsigned *>(p);
        h->skew_err_dev = static_cast<unsigned *>(d);
        *h->skew_err = 0;
    }
    const int sy = 8 / sk->tx;
    // The SIMD arbiter serves the older wave of a SIMD (waves 0..3) first: the
    // younger waves' bands are shorter so both finish together.  Measured
    // (round-3 skew_young sweeps, scripts/sweep_opts.py): two words per lane
    // 66-70 %, quads at depth 9 76-82 %.
    // half-wave-tile plans (16-turn launches of ramp-dominated bands): 60 %
    // (16384^2 87.6 vs 86.4 at 68, 83.7 at 55; profiles/r6b); whole tori on
    // full tiles 70 % (65536^2 128.7 vs 127.5-127.8 at 68, 126.4 at 74;
    // profiles/r6i); ring strips 68 % (their sweep is within its noise, r6d).
    // The pair rule's spaced shifts leave the older wave's
    // rate as it was and let the younger one issue in more of its gaps: whole
    // tori on full tiles 80 % (65536^2 144.2 vs 136.8 at 70, 139.5 at 86);
    // half tiles stay at 60 and ring strips at 68 (68-72 level; profiles/r8a)
    const int young = h->skew_young > 0 ? h->skew_young
                      : wpl == 4             ? 78
                      : sk->half             ? 60
                      : a.in.wrap > 0        ? (sk->pairs ? 80 : 70)
                                             : 68;
    for (int q = 0; q < 8; ++q) sk->wgt[q] = (q < sy && q * sk->tx >= 4) ? young : 100;
    sk->prio_young = h->skew_prio;
    sk->error = h->skew_err_dev;
    sk->trace = h->d_trace;
    return true;
}

// Halo mode with deep halos: one exchange of k * depth rows feeds k launches
// of `depth` turns.  Launch i (0-based) steps rows [-ext, rows + ext) with
// ext = (k - 1 - i) * depth, so it also rebuilds the next launch's halo rows
// from the wider halo (the trapezoid: output row -ext needs input rows
// -ext - depth .. , all inside the k * depth received rows).  The extension
// costs 2 * ext extra rows per launch; it saves k - 1 of every k exchanges.
int halo_launches(int rows, int depth, int64_t run) {
    const int64_t k = std::min<int64_t>({(int64_t)kHalo / depth, run, (int64_t)rows / depth});
    return (int)std::max<int64_t>(1, k);
}

// The next exchange of a halo-mode step: one exchange of k * d rows feeds k
// launches (resident: k super-steps) of d turns.  The one schedule of both
// golhip_step and golhip_halo_schedule (what tests/test_dist_gloo.py replays).
// Per-launch kernels take depth_plan's schedule; between exchanges the
// resident kernel runs full-depth super-steps cheaply and only a remainder
// goes to per-launch kernels, which are slow on strips this small: fewest
// short launches, greedily (1000 = 62 x 16 + 8, not 61 x 16 + 12 + 12).
HaloRun halo_next(int cap, int rows, bool resident, int64_t left) {
    DepthRun run = depth_plan(cap, left);
    if (resident) {
        const int d = largest_depth(std::min<int64_t>(cap, left));
        run = {d, left / d};
    }
    return {run.d, halo_launches(rows, run.d, run.n)};
}

// The resident kernel's depths: 4, 8, 16 and, at one word per lane, 32 (its
// instantiations); the per-launch depths 20, 24, 12, 9, 6 are not among them.
int persist_depth_for(golhip_t h, int wpl) {
    const int cap = std::min(h->persist_depth > 0 ? h->persist_depth : h->tb_depth, golk::persist_max_depth(wpl));
    for (int d : {32, 16, 8, 4})
        if (d <= cap) return d;
    return 1;
}

// The K1r plan of this torus at `wpl` words per lane (no side effects):
// one band per CU of at least D rows, both LDS buffers of a band in one
// workgroup's LDS, every workgroup resident.  Depth: the option, else 12
// (profiles/r4k-r4n sweeps: 8192^2 31.8 TCUPS at 12 vs 31.7 at 8 and 30.6 at
// 16; 5120^2 17.9 vs 17.0 and 17.7; 4096^2 13.4 vs 13.0 and 13.6), at most
// the row count.  False if K1r does not apply.
bool lds_fits(golhip_t h, int wpl, golk::LdsBandArgs *out) {
    if (h->lds_band == 0 || !h->torus() || h->W % 128 != 0 || (wpl == 2 && h->W % 64 != 0)) return false;
    if (h->nranks > 1) return false;
    // waves: 16 where a row's pairs fill whole waves at least twice and the
    // 1024 threads exactly (8192 wide: 40.9 vs 39.4 TCUPS at depth 10; 5120 /
    // 4096 wide lose a quarter with 16, their runs too short; 12288 wide, 960
    // of 1024 threads busy: 12.0 against K1p's 13.0 at 12288 x 2048;
    // profiles/r5m, r5n), else 8; depth 10 at 16 waves, else 12 (r5m: 8192^2
    // at 8 waves 39.8 / 39.4 / 38.9 at 10 / 12 / 14, 5120^2 21.2 / 21.6 / 21.2)
    const int P2 = h->Ww / 2;
    const int waves = h->lds_waves > 0 ? h->lds_waves
                      : (wpl == 2 && P2 % 64 == 0 && P2 >= 128 && 1024 % P2 == 0) ? 16 : 8;
    const int D = h->lds_depth > 0 ? h->lds_depth : std::min(waves == 16 ? 10 : 12, h->rows);
    if (h->rows < D || D < 1) return false;
    const int nt = 64 * waves;
    // auto: only where the rows' pairs (words) keep >= 90 % of the threads busy
    // (runs of whole columns: 512 / P runs each; 12288 x 2048 = 192 pairs a row
    // keeps 384 of 512 and ran 11.0 vs K1p's 13.0 TCUPS, while 1024^2 .. 8192^2,
    // 3072^2 and 8192 x 4096 run 1.3-2.1x K1p, profiles/r4x)
    if (h->lds_band < 0) {
        const int64_t P = h->Ww / wpl, units = P * std::max<int64_t>(1, nt / P);
        const int64_t slots = (units + nt - 1) / nt * nt;  // passes x threads
        if (10 * units < 9 * slots) return false;
    }
    // one progress word per band after d_sync's error word (2 dev_cu + 2 words)
    const int nb = std::min(std::min(h->cu_count, h->dev_cu) * h->lds_wg_cu, h->rows / D);
    if (nb < 1) return false;
    const int hmax = (h->rows + nb - 1) / nb;
    // the row stride: pairs always the two-plane row (Ww + 8, gol_kernels.hip K1r)
    const int stride = golk::lds_band_stride(h->Ww, wpl, nt);
    const int64_t bytes = golk::lds_band_lds_bytes(hmax, D, stride);
    if (bytes > 160 * 1024 - 256) return false;  // (the kernel's few static LDS bytes)
    const int slot = (wpl == 2 ? 1 : 0) + (nt == 1024 ? 2 : 0);
    int &bpc = h->lds_bpc[slot];
    if (bpc == 0 || h->lds_bpc_bytes[slot] != bytes || h->lds_bpc_stride[slot] != stride) {
        bpc = std::max(0, golk::lds_band_blocks_per_cu(wpl, nt, stride, bytes));
        h->lds_bpc_bytes[slot] = bytes;
        h->lds_bpc_stride[slot] = stride;
    }
    if ((int64_t)nb > (int64_t)bpc * h->cu_count) return false;
    if (out) {
        out->Ww = h->Ww;
        out->rows = h->rows;
        out->nb = nb;
        out->D = D;
        out->hmax = hmax;
        out->xcd = h->lds_xcd;
        out->nt = nt;
        out->stride = stride;
        out->rt_stride = h->lds_stride ? 0 : 1;
        out->fault = h->resident_fault != 0;
        out->pre = h->lds_pre;
        // the SIMD arbiter's age order, where whole waves share a run (a row's
        // pairs a multiple of 64): 16 waves (4 ranks) 60 %, 8 waves 70 %
        // (profiles/r5z: 8192^2 40.2 -> 43.8 TCUPS, 4096^2 17.1 -> 17.8); runs
        // that straddle waves stay equal (5120^2 +1 % at 80, 2048^2 -5 %)
        const bool whole = wpl == 2 && P2 % 64 == 0;
        out->age = h->lds_age > 0 ? h->lds_age : !whole ? 100 : waves == 16 ? 60 : 70;
    }
    return true;
}

}  // namespace gh

using namespace gh;

extern "C" {

int golhip_halo_schedule(int32_t strip_rows, int32_t tb_depth, int32_t resident, int64_t turns_left,
                         int32_t *depth, int32_t *launches) {
    if (!depth || !launches || strip_rows <= 0 || tb_depth < 1 || tb_depth > GOLHIP_MAX_TB_DEPTH || turns_left < 1)
        return fail(GOLHIP_EINVAL, "bad halo schedule request");
    const HaloRun hr = halo_next(std::min(tb_depth, strip_rows), strip_rows, resident != 0, turns_left);
    *depth = hr.d;
    *launches = hr.k;
    return GOLHIP_OK;
}

int golhip_depth_schedule(int32_t cap, int32_t pair_tail, int64_t turns_left, int32_t *depth, int64_t *launches) {
    if (!depth || !launches || cap < 1 || cap > GOLHIP_MAX_TB_DEPTH || turns_left < 1 || (pair_tail && cap != 18))
        return fail(GOLHIP_EINVAL, "bad depth schedule request");
    const DepthRun run = depth_plan(cap, turns_left, pair_tail != 0);
    *depth = run.d;
    *launches = run.n;
    return GOLHIP_OK;
}

int64_t golhip_launch_cost(int32_t depth, int32_t pair_kernel) {
    if (depth < 1 || depth > GOLHIP_MAX_TB_DEPTH) return -1;
    return launch_cost(depth, pair_kernel != 0);
}

int golhip_skew_span(const golhip_skew_span_in_t *in, int32_t *k_lo, int32_t *k_hi) {
    if (!in || !k_lo || !k_hi || in->depth < 4 || in->depth > GOLHIP_MAX_TB_DEPTH || in->eb < in->ab || in->dr < 0 || in->row_words < 1)
        return fail(GOLHIP_EINVAL, "bad skew span request");
    const golk::SkewSpan s = golk::skew_interior_span(golk::SkewSpanIn{
        in->ab, in->eb, in->depth, in->self != 0, in->pair != 0, in->off, in->wrap, in->rmax, in->half != 0, in->dr, in->row_words,
        in->counts != 0, in->enabled != 0});
    *k_lo = s.k_lo;
    *k_hi = s.k_hi;
    return GOLHIP_OK;
}

int golhip_skew_interior_plan(golhip_t h, int32_t depth, int32_t ext, int32_t counts, int64_t *interior_bodies,
                              int64_t *main_bodies) {
    if (int rc = check(h)) return rc;
    if (!interior_bodies || !main_bodies || depth < 1 || ext < 0) return fail(GOLHIP_EINVAL, "bad skew interior request");
    std::lock_guard<std::mutex> g(h->mu);
    *interior_bodies = *main_bodies = 0;
    const bool halo = h->halo_mode();
    if (ext > 0 && !halo) return fail(GOLHIP_EINVAL, "extended rows: strips only");
    golk::StepArgs a = step_args(h, nullptr, halo);
    if (ext > 0) {  // launch_rows' deep-halo extension
        a.rows_out = h->rows + 2 * ext;
        a.in.off = kHalo - ext;
        a.count_lo = ext;
        a.count_hi = ext + h->rows;
    }
    golk::SkewArgs sk{};
    const int wpl = wpl_for(h);
    // (a whole torus' own steps run 12 / 15 / 16 turns on the pair kernel)
    h->pair_tail_step = !halo && ext == 0 && pair_tail_on(h);
    const bool planned = skew_plan(h, depth, wpl, a, &sk);
    h->pair_tail_step = false;
    if (!planned) return GOLHIP_OK;  // no K1w launch at this depth: no bodies
    const int sy = 8 / sk.tx, L = sk.half ? a.rows_out / 2 : a.rows_out, B = sk.pairs ? 6 : 3;
    for (int stack = 0; stack < sk.nst; ++stack)
        for (int pos = 0; pos < sy; ++pos) {
            const golk::SkewBand b = golk::skew_band(L, sk.nst, stack, sy, pos, sk.wgt, sk.hcap, depth, sk.pairs != 0);
            const golk::SkewSpan s = golk::skew_interior_span(golk::SkewSpanIn{
                b.ab, b.eb, depth, b.bottom, sk.pairs != 0, a.in.off, a.in.wrap, a.in.rmax, sk.half != 0, L, a.Ww,
                counts != 0 && a.count_lo < a.count_hi, sk.interior != 0});
            const int k0 = golk::skew_main_start(depth, sk.pairs != 0), k1 = golk::skew_main_end(b.eb - b.ab, depth, b.bottom);
            *interior_bodies += (int64_t)(s.k_hi - s.k_lo) / B * sk.tiles_x;
            *main_bodies += (int64_t)(std::max(k1 - k0, 0) + B - 1) / B * sk.tiles_x;
        }
    return GOLHIP_OK;
}

int golhip_halo_plan(int32_t width, int32_t strip_rows, int32_t nranks, int32_t rank, int32_t depth,
                     golhip_halo_plan_t *out) {
    if (!out || width <= 0 || strip_rows <= 0 || nranks < 1 || rank < 0 || rank >= nranks || depth < 1 ||
        depth > GOLHIP_HALO_ROWS || depth > strip_rows)
        return fail(GOLHIP_EINVAL, "bad halo plan request");
    halo_plan(strip_rows, nranks, rank, depth, (width + 31) / 32, out);
    return GOLHIP_OK;
}

}  // extern "C"
