/*
 * golhip.h — C-ABI of libgolhip.so, the MI355X engine behind gol.Run.
 *
 * The reference's hot path is the per-turn loop of
 *   gol/distributor.go:93-173  distributor(): serial calculateNextState (:350-379)
 *                              or the worker pool worker/workerWorld (:304-347),
 *                              both over checkNeighbour (:382-417);
 * with its side channels
 *   gol/distributor.go:212-220 initializeAliveCells  -> CellFlipped events
 *   gol/distributor.go:420-432 calculateAliveCells   -> FinalTurnComplete.Alive,
 *                                                       AliveCellsCount (:283-302)
 *   gol/distributor.go:66-80   world fill from the io goroutine (ioInput)
 *   gol/distributor.go:180-191 final PGM stream (ioOutput), also s/q (:229-261).
 * The reference has no FFI of its own (pure Go); these entry points are what a
 * cgo shim in gol/distributor.go binds in place of those functions
 * (INTEGRATION.md shows the binding).  Plain pointers and sizes only.
 *
 * Board model: a width x height torus, rows are y (0..height-1), columns x.
 * Byte boards are row-major height x width, alive <=> byte == 255 (the
 * reference's test `world[x][y] == 255`, distributor.go:363, :411); byte
 * outputs are 0 / 255.  Bit boards are row-major, ceil(width/32) uint32 words
 * per row, cell (y, x) = bit x%32 of word x/32 (padding bits zero).
 *
 * Conventions: every function returns 0 (GOLHIP_OK) or a negative GOLHIP_E*
 * code and sets a thread-local message for golhip_last_error().  Caller-owned
 * buffers are never retained past the call (cgo pointer rules).  One handle is
 * driven by one engine thread; golhip_turn and golhip_alive_count may be
 * called concurrently from another thread (the reference's ticker, :283-302)
 * and return a (turn, count) pair that belongs together.
 *
 * The handle as a state machine: oracle/handle_model.py restates this header
 * as a numpy model of one handle (and of a group of strips) -- the board, the
 * turn, the flip list kept, the checkpoints and images in flight -- and
 * answers every call with the value or the code documented here; where this
 * header is silent the model says nothing.  tests/test_gpu_sequences.py draws
 * seeded call sequences from the model's weighted tables (loads, stamps,
 * steps, flip and view streams, plan changes between steps, observers, jobs
 * in flight, refused calls) and compares handle and model after every call;
 * its last test requires that the committed seeds took every kernel family
 * (K1g, K1, K1w, the pair rule, K1r, K1p, the padded torus, K5, K5r), moved
 * the words per lane of a loaded board up and down, and put a stamp, a clear
 * and a step between a job's begin and its wait.
 *
 * Patterns go both ways: "patterns" below puts a rectangle of cells (bit
 * words, an RLE file, a PGM) anywhere on the torus, "saving patterns" reads
 * any rectangle back, finds the smallest box around the alive cells and writes
 * either as an RLE file whose header names the board's rule -- the way to take
 * home what a pattern became on a board too large to save as an image.  The
 * model of oracle/ does not know the saving calls: they are observers, checked
 * by tests/test_gpu_extract.py.
 */
#ifndef GOLHIP_H
#define GOLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOLHIP_OK 0
#define GOLHIP_EINVAL (-1)  /* bad argument (size, pointer, state)            */
#define GOLHIP_EHIP (-2)    /* HIP runtime error                              */
#define GOLHIP_ENOMEM (-3)  /* device or host allocation failed               */
#define GOLHIP_ERANGE (-4)  /* caller buffer too small (required size is set) */
#define GOLHIP_ERCCL (-5)   /* RCCL error                                     */
#define GOLHIP_ECORRUPT (-6) /* checkpoint file damaged: header check, size, digest or count */

/* golhip_create flags */
#define GOLHIP_FLAG_TIMING 0x1u /* time every step kernel with HIP events     */

#define GOLHIP_UNIQUE_ID_BYTES 128 /* == sizeof(ncclUniqueId)                 */
#define GOLHIP_MAX_TB_DEPTH 32     /* max turns fused in one step launch      */
#define GOLHIP_HALO_ROWS 128       /* halo rows above/below a strip buffer    */

typedef struct golhip golhip;
typedef golhip *golhip_t;

typedef struct golhip_perf {
    int64_t turns;            /* turns completed since the last load/fill     */
    int64_t step_launches;    /* per-launch step kernels (gol_tb_kernel) since golhip_perf_reset */
    int64_t step_turns;       /* turns run by those launches                  */
    double step_kernel_ms;    /* their summed device time (GOLHIP_FLAG_TIMING)*/
    int64_t persist_launches; /* persistent step kernels (gol_persist_kernel) */
    int64_t persist_turns;    /* turns run by those                           */
    double persist_kernel_ms; /* their summed device time (GOLHIP_FLAG_TIMING)*/
    int64_t cell_updates;     /* width * local rows * all stepped turns       */
    int64_t alg_bytes;        /* 0.25 B per cell-update (1 bit in + 1 bit out)*/
    int64_t halo_bytes;       /* bytes sent to neighbour ranks                */
    int32_t tb_depth;         /* most turns one step launch fuses (the setting,
                                 capped by the kernel's words per lane)       */
    int32_t rows_per_wave;    /* rows streamed per wavefront (full-depth launch)*/
    int32_t kernel_variant;   /* 0 = generic (width % 32 != 0), 1 = bit-sliced, 3 = skewed
                                 band stacks, 4 = resident LDS bands, 5 = the rule kernel
                                 (K11, golhip_set_rule; any width), 6 = the plane kernel
                                 (K15, golhip_set_topology; any width); after a padded
                                 step: the wide board's                       */
    int32_t words_per_lane;   /* 1, 2 (interleaved pairs) or 4 (quads); 0 generic
                                 (width % 32 != 0 off the plane kernel)       */
    int64_t persist_fallbacks; /* resident launches that timed out (not all workgroups
                                  co-resident) and were re-run on per-launch kernels */
    int64_t flip_launches;    /* fused turn + flip-list kernels (one turn each)  */
    int64_t flip_entries;     /* flip-list entries copied to the caller          */
    double flip_kernel_ms;    /* their summed device time (GOLHIP_FLAG_TIMING)   */
    int64_t flip_fallbacks;   /* flip batches re-run in ticket order (a block waited on a
                                 predecessor that was not resident)                */
    int32_t persist_depth;    /* turns per super-step of the resident kernel (its
                                 depths stop at 16 for two words per lane)       */
    int32_t reserved0;
    int64_t pad_launches;     /* seam refreshes of the padded torus, one per launch of the
                                 wide board (golhip_set_pad_step; the offset of the
                                 retired split_launches / reserved1)             */
    int64_t skew_launches;    /* of step_launches, those that ran skewed band
                                 stacks (gol_skew_kernel, kernel_variant 3)     */
    int64_t halo_exchanges;   /* halo exchanges posted (RCCL ring)               */
    double halo_ms;           /* their summed time on the stream they ran on
                                 (GOLHIP_FLAG_TIMING)                           */
    int64_t rule_launches;    /* of step_launches, those on the rule kernels (K11,
                                 kernel_variant 5; K15 on a plane, 6; the offset of the retired
                                 overlap_launches / reserved2)                   */
    int64_t skew_half_launches; /* of skew_launches, those on half-wave tiles    */
    int64_t lds_launches;     /* of persist_launches, those that ran resident LDS
                                 bands (gol_lds_band_kernel, kernel_variant 4)  */
    int64_t pair_launches;    /* of skew_launches, those on the pair rule (option
                                 "skew_pairs": 8 LUTs a word-turn; round 6)     */
    int64_t pair_turns;       /* turns run by those                              */
    int64_t flip_resident_launches; /* flip-stream batches run as one resident launch
                                 (K5r, flip_overlap 2; round 6); their turns count in
                                 flip_launches, their time in flip_kernel_ms     */
    int64_t view_frames;      /* frames rendered by the view kernels (K7)          */
    double view_kernel_ms;    /* their summed device time (GOLHIP_FLAG_TIMING)   */
} golhip_perf_t;

/* ---- library ---------------------------------------------------------- */
const char *golhip_version(void);
/* The build's kernel tuning macros, "NAME=value ..." (A/B builds override
 * them; the shipped library is built with the defaults).  Measurement. */
const char *golhip_build_info(void);
const char *golhip_last_error(void);
int golhip_device_count(int32_t *n);

/* Page-locked host memory that the device writes directly (hipHostMalloc,
 * mapped).  A golhip_flip_stream whose `out` lies inside such a buffer gets
 * its entries written by the kernels themselves over PCIe (each turn's list
 * by the next launch's copy blocks while that turn computes): no host-side
 * copy after the batch.  Go callers use it as C memory (unsafe.Slice). */
int golhip_host_alloc(uint64_t bytes, void **out);
int golhip_host_free(void *p);
/* Measurement (no reference counterpart): the host link's rates into a
 * buffer of golhip_host_alloc's kind -- a kernel streaming coalesced 16-byte
 * stores into it (what the event-stream kernel's entries ride) and the DMA
 * engine's device-to-host copy -- over `bytes` (>= 4096, a multiple of 16),
 * `reps` passes each after one warm pass, in GB/s (1e9 B/s). */
int golhip_host_link_probe(int32_t device, uint64_t bytes, int32_t reps, double *kernel_write_gbps,
                           double *dma_d2h_gbps);

/* ---- handles ---------------------------------------------------------- */
/* Whole width x height torus on one device.  Replaces the world allocation
 * of distributor.go:66-69. */
int golhip_create(int32_t width, int32_t height, int32_t device, uint32_t flags, golhip_t *out);

/* Row strip [row0, row0 + rows) of a width x height torus (multi-GPU row-strip
 * decomposition, README halo-exchange extension).  Its halo rows come from
 * the neighbouring strips through golhip_comm_init (one process per GPU, RCCL)
 * or golhip_group_step (several strips driven by one process). */
int golhip_create_strip(int32_t width, int32_t height, int32_t row0, int32_t rows, int32_t device,
                        uint32_t flags, golhip_t *out);
int golhip_destroy(golhip_t h);

/* Run on a caller-provided hipStream_t (e.g. torch.cuda.current_stream()). */
int golhip_set_stream(golhip_t h, void *hip_stream);
void *golhip_stream(golhip_t h);

/* Tuning: turns fused per launch (1..GOLHIP_MAX_TB_DEPTH, default 20; capped
 * per kernel: 32 at one word per lane, 20 at two (16 for the resident
 * kernel), 8 at four) and rows streamed
 * per wavefront (0 = automatic, the default: sized from the CU count and the
 * kernel's occupancy).  Results never depend on them. */
int golhip_set_tb_depth(golhip_t h, int32_t turns);
int golhip_set_rows_per_wave(golhip_t h, int32_t rows);
/* Named engine options; results never depend on them.
 *
 * Product options (no consent needed):
 * "wpl" (default 0 = auto): words per lane, 1, 2 or 4 (2 and 4 run on the
 *   interleaved pair / quad layouts, converted at the I/O boundary; 4 needs
 *   width % 128 == 0);
 * "persistent" (-1 = auto: off where the skewed band stacks fill the CUs,
 *   else on for buffers of at most 64 MiB; 1 on, 0 off): resident kernels
 *   (K1p, K1r) for long runs on a whole torus, never in a multi-rank ring --
 *   0 keeps a shared GPU free of kernels that wait on co-resident workgroups;
 * "lds_band" (-1 = auto, 1, 0): resident LDS bands (K1r, W % 128 == 0);
 * "skew" (1; 2 always, 0 off): skewed band stacks (K1w) for per-launch steps;
 * "timing" (GOLHIP_FLAG_TIMING after creation: per-launch HIP events);
 * "persist_timeout_us" (1000000): how long a resident workgroup waits for a
 *   neighbour before the launch is abandoned (the board is restored and the
 *   step re-run on per-launch kernels, perf.persist_fallbacks);
 * "force_halo" (0): after golhip_comm_init with one rank, run a whole board
 *   through the multi-GPU path as a one-rank RCCL ring.
 *
 * A/B tuning knobs of the kernel plans, refused without GOLHIP_TUNING=1 (or
 * GOLHIP_MEASUREMENT=1); the defaults are the measured plans:
 * persist_depth, persist_waves, persist_half, persist_wg_tx, paired_bands,
 * dummy_rows, trace (golhip_persist_trace), cu_count, fill_skip, skew_young,
 * skew_hcap, skew_prio, skew_half, skew_tx, lds_depth, lds_waves, lds_wg_cu,
 * lds_age, lds_pre, lds_stride, lds_xcd, skew_pairs (bit 1: tori and strips on
 * full-width K1w tiles run 18 turns a launch with the pair rule, 8 LUTs a
 * word-turn; bit 4: half-wave tile plans too; bit 2: quads at 8 on the pair
 * rule; default 5), skew_interior (1, the default: that kernel's main loop
 * runs the rows between a band's first and last stored rows, where the row map
 * neither wraps nor clamps, through a body without the per-row decisions, in
 * launches that count nothing; 0: the general body throughout; same results,
 * DESIGN.md 5.20; not listed by golhip_build_info()),
 * flip_overlap (how a golhip_flip_stream into golhip_host_alloc memory
 * delivers the lists: 2 (the default), boards of at least 64 K words run the
 * batch's turns as one resident launch whose copy blocks move each turn's
 * list to the host while the next turns compute, the rest (and whatever that
 * launch cannot run) as 1; 3, the resident launch at any size; 1, each
 * launch's copy blocks move the previous turn's list; 0, the turn's blocks
 * store their entries there).  Environment overrides for handles a caller
 * creates itself (GOLHIP_TUNING=1): GOLHIP_FLIP_OVERLAP=0..3, and
 * GOLHIP_FLIP_CP_GROUPS=1..8, the resident launch's copy-block groups (each
 * group copies every n-th turn; default 4).
 *
 * Measurement only, refused without GOLHIP_MEASUREMENT=1 (WRONG results by
 * design): "halo_skip" (post no halo exchange), "flip_debug" 1-3.
 *
 * Test hooks, refused without GOLHIP_TEST_HOOKS=1 (exact results, forced
 * failure paths): "resident_fault" (1: the resident kernels' band /
 * workgroup 0 never reports in any launch, 2: only in a step's first
 * resident launch; the neighbours' bounded waits time out and the step is
 * restored and re-run), "resident_max_turns" (lowers the turns one resident
 * launch takes, so a step runs several), "flip_debug" 4, "rule_kernel" (1: a
 * handle with Conway's rule steps on the rule kernel K11 too, on its static
 * policy; 2: K11's dynamic policy for every rule, those with a static instance
 * included; same boards either way, so the golden boards judge both policies;
 * not listed by golhip_build_info()).
 *
 * golhip_build_info() lists the three consent sets and the product options.
 * Retired (refused as unknown keys): "split", "lds_split", "skew_nst",
 * "age_split", "overlap". */
int golhip_set_option(golhip_t h, const char *key, int64_t value);
/* The padded torus: a whole torus without a communicator whose width is no
 * multiple of 32 may step on the fast per-launch kernels as a slightly wider
 * torus (width rounded up to a multiple of 64 past width + 64) whose extra
 * columns are ghost copies of real ones, refreshed before every launch; the
 * board of this handle is whole again when golhip_step returns.  Results never
 * depend on it.  mode -1 (the default): where it measured faster than the
 * any-width kernel, by the board's cells and the turns of the call (DESIGN.md
 * 5.17), falling back to that kernel if the wide board cannot be allocated;
 * 0: never; 1: always (golhip_step then fails with GOLHIP_ENOMEM if the wide
 * board cannot be allocated) -- mode 1 is GOLHIP_EINVAL on a strip, a ring or
 * a handle whose width is a multiple of 32 (-1 and 0 are accepted there and
 * change nothing).  It concerns golhip_step alone (and what
 * steps through it): golhip_flip_stream, golhip_step_flips and
 * golhip_group_flip_stream run every width on the fused turn + list kernel,
 * which closes the row seam itself (no wide board, pad_launches stays 0); the
 * strips of a group have golhip_group_set_pad_step, and a ring's steps keep
 * the any-width kernel.  perf: pad_launches. */
int golhip_set_pad_step(golhip_t h, int32_t mode);

/* ---- Life-like rules -------------------------------------------------- */
/* A rule is two 9-bit masks: bit n of `birth`, a dead cell with n alive
 * neighbours (of 8, the centre excluded) comes alive; bit n of `survive`, an
 * alive cell with n stays alive.  Conway's B3/S23 is birth 0x008, survive
 * 0x00C, the rule of every new handle.  B0 is legal (well defined on a torus).
 *
 * golhip_rule_parse reads "B<digits>/S<digits>" in either letter case, either
 * half possibly empty ("B2/S"), or the legacy "<survive digits>/<birth digits>"
 * ("23/3"); white space around it, digits 0..8 in any order, none repeated.
 * Anything else (a digit 9, no '/', Generations "/C", non-totalistic
 * suffixes) is GOLHIP_EINVAL with a message naming the fault.
 * golhip_rule_format writes the canonical "B36/S23" (digits ascending, NUL
 * terminated); GOLHIP_ERANGE if `cap` bytes do not hold it, GOLHIP_EINVAL for a
 * mask above 0x1FF. */
int golhip_rule_parse(const char *text, uint32_t *birth, uint32_t *survive);
int golhip_rule_format(uint32_t birth, uint32_t survive, char *out, uint64_t cap);
/* The rule of the turns enqueued from now on (masks above 0x1FF: GOLHIP_EINVAL).
 * Any time on a handle without a communicator; the board, the turn, the kept
 * count and the flip list stay.  A handle with another rule than Conway's steps
 * on the rule kernel (K11, canonical words, up to 16 turns a launch; widths
 * that are no multiple of 32 through the padded torus or one turn a launch),
 * never on the resident or skewed kernels, and its flip streams take one turn
 * and one three-pass compaction a turn (same contract) unless
 * golhip_set_rule_flips sends them through the fused kernel.  Every other call
 * works on it unchanged.  The strips of one group must all have the same rule
 * (every call that takes a group: GOLHIP_EINVAL otherwise).
 * Rings: a handle with a communicator (golhip_comm_init, one-rank rings and
 * golhip_test_ring_init's included) refuses every rule but Conway's, and
 * golhip_comm_init / golhip_test_ring_init refuse a handle that has another:
 * the ranks of a ring could disagree on the rule and nobody would notice. */
int golhip_set_rule(golhip_t h, uint32_t birth, uint32_t survive);
int golhip_rule(golhip_t h, uint32_t *birth, uint32_t *survive);
/* How golhip_flip_stream and golhip_step_flips run on a handle with another
 * rule than Conway's.  mode 0 (the default): one step-kernel launch, a
 * three-pass compaction and two host synchronisations a turn.  mode 1: one
 * launch a turn of K14, the fused turn + list kernel with the rule as a
 * policy (a static instance for the named rules, the dynamic policy for every
 * other), with everything the fused kernel gives Conway: one host round trip
 * a batch, lists written into golhip_host_alloc memory by the launches' copy
 * blocks ("flip_overlap" 2 runs as 1: K14 has no resident form), the
 * co-residency fallback.  Same lists, counts, turns_done and return codes
 * either way.  Any other value: GOLHIP_EINVAL, nothing changed.  Legal any
 * time; the board, the turn, the kept count and the flip list stay.  A handle
 * with Conway's rule keeps its own kernels whatever the mode, and so does a
 * strip of 2^32 - 4096 words or more its per-turn path.
 * golhip_group_flip_stream takes the fused per-strip path when every strip of
 * the group has mode 1 and the per-turn path otherwise.  perf: flip_launches
 * and flip_entries count K14 as they count Conway's kernel; rule_launches and
 * step_launches do not move on a mode-1 stream. */
int golhip_set_rule_flips(golhip_t h, int32_t mode);
int golhip_rule_flips(golhip_t h, int32_t *mode);

/* ---- Topology: torus or bounded plane ---------------------------------- */
/* GOLHIP_TOPOLOGY_TORUS (the default of every new handle): the board's edges
 * meet, as everywhere above.  GOLHIP_TOPOLOGY_PLANE: Golly's bounded plane
 * "B3/S23:P512,512": every cell outside [0, W) x [0, H) is dead for ever, at
 * every turn.  A margin of dead cells cannot give that (a cell born in the
 * margin feeds the board's edge a turn later), so a plane handle steps on K15,
 * the rule kernel with the outside forced dead inside every fused turn: any
 * rule (Conway's on its static policy), ANY width at up to 16 turns a launch
 * on canonical words (a plane has no row seam: no padded torus, pad_launches
 * stays 0), never on the resident or skewed kernels.  perf: kernel_variant 6;
 * its launches count in rule_launches.
 * golhip_set_topology: any time on a handle without a communicator (a handle
 * with one, golhip_test_ring_init's included, refuses the plane; the torus is
 * always accepted); the board, the turn, the kept count and the flip list
 * stay, and the turns enqueued from now on run on the new topology.  A handle
 * with golhip_set_pad_step 1 refuses the plane, and a plane handle refuses
 * golhip_set_pad_step 1 (ghost columns are copies; a plane has none).  The
 * flip streams of a plane handle take the per-turn path (one K15 turn and one
 * three-pass compaction a turn) whatever golhip_set_rule_flips says: same
 * lists, counts and return codes.  The strips of one group must all have the
 * same topology (every call that takes a group: GOLHIP_EINVAL otherwise).
 * Count, hash, view, image, checkpoint, stamp and extract do not look at the
 * topology (a stamp or an extract that crosses an edge still wraps);
 * golhip_alive_box returns the plain min / max box on a plane handle, and
 * golhip_save_rle on one writes "rule = <B/S>:P<W>,<H>", so the file reopens
 * bounded (golhip_pattern_write takes no handle and writes the plain rule).
 * A checkpoint keeps no topology, as it keeps no rule: a resume sets it again. */
#define GOLHIP_TOPOLOGY_TORUS 0
#define GOLHIP_TOPOLOGY_PLANE 1
int golhip_set_topology(golhip_t h, int32_t topology);
int golhip_topology(golhip_t h, int32_t *topology);
/* golhip_rule_parse with Golly's bounded-grid suffix: what golhip_rule_parse
 * takes, then optionally ":T<w>,<h>" (torus) or ":P<w>,<h>" (plane), the letter
 * in either case, w and h in 1 .. 2^31 - 1.  Without a suffix *topology is
 * GOLHIP_TOPOLOGY_TORUS and both bounds are 0.  A bound of 0 (Golly's infinite
 * dimension), a missing bound, another topology letter or anything behind the
 * bounds is GOLHIP_EINVAL with a message naming the fault.  golhip_rule_parse
 * itself goes on refusing the suffix.
 * golhip_rule_format_ex is the inverse: "B3/S23:P512,512"; with both bounds 0
 * and the torus, golhip_rule_format's text.  GOLHIP_EINVAL for a plane without
 * bounds, one bound of 0, a negative bound or another topology. */
int golhip_rule_parse_ex(const char *text, uint32_t *birth, uint32_t *survive, int32_t *topology, int32_t *bw,
                         int32_t *bh);
int golhip_rule_format_ex(uint32_t birth, uint32_t survive, int32_t topology, int32_t bw, int32_t bh, char *out,
                          uint64_t cap);

/* ---- multi-GPU -------------------------------------------------------- */
/* RCCL ring of strips: rank r's neighbours are r-1 (rows above) and r+1
 * (rows below), mod nranks (toroidal wrap).  id comes from rank 0's
 * golhip_comm_unique_id, broadcast by the caller. */
int golhip_comm_unique_id(uint8_t id[GOLHIP_UNIQUE_ID_BYTES]);
int golhip_comm_init(golhip_t h, const uint8_t id[GOLHIP_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank);
/* The ring as the communicator itself reports it (ncclCommCount /
 * ncclCommUserRank) and the strip rows every rank plans from (the ring's
 * smallest strip, agreed at golhip_comm_init).  Without a comm: 1, 0, and
 * this handle's rows.  No reference counterpart (measurement). */
int golhip_comm_info(golhip_t h, int32_t *nranks, int32_t *rank, int32_t *ring_rows);

/* Test hook, refused without GOLHIP_TEST_HOOKS=1 (no reference counterpart):
 * make a strip handle rank `rank` of an `nranks` ring whose halo exchange
 * runs through `fn` instead of RCCL, so that two processes can drive a ring
 * on one device.  At each exchange the library stages the strip's two send
 * blocks (its first and last `bytes / 4 / row words` rows beyond the halo
 * plan's send rows) in pinned memory and calls fn(user, prev_rank, next_rank,
 * send_up, send_down, recv_top, recv_bottom, bytes): fn must fill recv_top
 * with prev_rank's send_down and recv_bottom with next_rank's send_up, and
 * return 0.  Everything else (golhip_halo_schedule's rounds, the deep-halo
 * launches, the kernels) is the RCCL ring's; ring_rows is the ring's smallest
 * strip (golhip_comm_init agrees it by allreduce; here the caller passes it).
 * golhip_alive_count_global's allreduce runs through the same fn: prev_rank =
 * next_rank = -1, send_up = this rank's uint64 count, recv_top = where the
 * ring's sum goes, bytes = 8 (send_down, recv_bottom null). */
typedef int (*golhip_test_transport_fn)(void *user, int32_t prev_rank, int32_t next_rank, const void *send_up,
                                        const void *send_down, void *recv_top, void *recv_bottom, int64_t bytes);
int golhip_test_ring_init(golhip_t h, int32_t nranks, int32_t rank, int32_t ring_rows, golhip_test_transport_fn fn,
                          void *user);

/* Steps n strips (ring order = array order) driven from one process; halos
 * move with peer/device copies.  Same semantics as golhip_step on each. */
int golhip_group_step(golhip_t *hs, int32_t n, int64_t nturns);
/* golhip_group_step with golhip_step's want_flips: every strip keeps the flip
 * list of the last turn for golhip_flips (global coordinates; concatenated in
 * strip order they are the board's row-major list).  Used by gol.Run with
 * GOL_NGPU / GOL_STRIPS (the row-strip decomposition behind the drop-in). */
int golhip_group_step_ex(golhip_t *hs, int32_t n, int64_t nturns, int32_t want_flips);
/* Padded strips: golhip_set_pad_step for the strips of a group.  Every strip
 * of a group whose width is no multiple of 32 may step as a wide strip of the
 * padded torus (its halo rows too: one deep-halo exchange of wide rows, then
 * launches of up to 32 turns, the ghosts of the rows a launch reads refreshed
 * before it); every strip's board is whole again when golhip_group_step[_ex]
 * returns.  All strips pad or none does, decided once a call from the mode
 * kept on strip 0: -1 (the default) where it measured faster than the
 * any-width kernel, by the board's cells and the turns of the call (DESIGN.md
 * 5.17), falling back to that kernel for the group's life if a wide strip
 * cannot be allocated; 0: never; 1: always (the step then fails with
 * GOLHIP_ENOMEM if a wide strip cannot be allocated) -- GOLHIP_EINVAL for a
 * width that is a multiple of 32 or a strip with a communicator.  A
 * want_flips step runs its last turn on the any-width kernel.  perf:
 * pad_launches, one per launch of a wide strip. */
int golhip_group_set_pad_step(golhip_t *hs, int32_t n, int32_t mode);

/* Halo plan used by both transports (exposed for tests): rows this strip
 * sends up/down and receives for an exchange of `depth` rows
 * (1 <= depth <= min(GOLHIP_HALO_ROWS, strip_rows)). */
typedef struct golhip_halo_plan {
    int32_t prev_rank, next_rank;   /* ring neighbours                       */
    int32_t send_up_row, recv_top_row;     /* physical buffer rows             */
    int32_t send_down_row, recv_bottom_row;
    int32_t rows;                   /* = depth                               */
    int64_t bytes;                  /* per message                            */
} golhip_halo_plan_t;
int golhip_halo_plan(int32_t width, int32_t strip_rows, int32_t nranks, int32_t rank, int32_t depth,
                     golhip_halo_plan_t *out);
/* Exchange schedule of a strip, exactly as golhip_step runs it: each
 * exchange moves launches * depth halo rows, then `launches` step launches of
 * `depth` turns follow; launch i (0-based) steps rows [-e, strip_rows + e),
 * e = (launches - 1 - i) * depth, so it rebuilds the next launch's halos from
 * the deeper exchanged ones (kernel-side rows, W % 32 == 0; other widths run
 * one turn per launch).  tb_depth: the most turns a launch may fuse (the
 * setting capped by the kernel's words per lane, golhip_perf tb_depth);
 * resident != 0: the strip runs the resident kernel between exchanges
 * (option "persistent", on by default for strips of <= 64 MiB), which takes
 * full-depth super-steps greedily instead of the balanced launch plan. */
int golhip_halo_schedule(int32_t strip_rows, int32_t tb_depth, int32_t resident, int64_t turns_left,
                         int32_t *depth, int32_t *launches);
/* The launch schedule of a step that is no strip's (exposed for tests): the
 * next run of `launches` launches of `depth` turns for turns_left turns at
 * most `cap` turns a launch, exactly as golhip_step plans it.  pair_tail != 0
 * (cap 18 only): the plan of a whole torus on the pair rule's full-width
 * tiles, whose last launches may take the pair kernel's remainder depths 12,
 * 15 and 16 and are ranked by golhip_launch_cost; 0: every other plan. */
int golhip_depth_schedule(int32_t cap, int32_t pair_tail, int64_t turns_left, int32_t *depth, int64_t *launches);
/* That ranking's estimate of one launch of `depth` turns on the pair kernel
 * (pair_kernel != 0) or on the 9-LUT stages: (depth + ramp) x issue slots a
 * word-turn, in tenths of a turn-slot.  -1: bad depth. */
int64_t golhip_launch_cost(int32_t depth, int32_t pair_kernel);
/* The interior span of one band of a skewed-stack launch (exposed for tests;
 * DESIGN.md 5.20): the main-loop pushes [k_lo, k_hi), whole loop bodies, in
 * which the band's input rows [ab, eb) neither wrap (wrap; 0: no wrap) nor
 * clamp (rmax) through the row map (off), every stored row lies inside the
 * band and nothing is counted, exactly as the kernel decides it.  self: the
 * stack's bottom band; pair: the pair rule's bodies of six rows (else three);
 * half: the wave's upper lanes run the same band dr rows further down (both
 * halves within 2 GiB of one base, at row_words words a row); counts:
 * the launch counts alive cells; enabled: option "skew_interior".  Empty
 * (k_lo = k_hi) when there is none. */
typedef struct golhip_skew_span_in {
    int32_t ab, eb, depth, self, pair;
    int32_t off, wrap, rmax;
    int32_t half, dr, row_words, counts, enabled;
} golhip_skew_span_in_t;
int golhip_skew_span(const golhip_skew_span_in_t *in, int32_t *k_lo, int32_t *k_hi);
/* The same over every wave of the skewed-stack launch of `depth` turns this
 * handle would run now (a strip: over its rows extended by ext on either
 * side; counts != 0: a launch that counts): main-loop bodies inside an
 * interior span, and all main-loop bodies.  Both 0 where no such launch
 * exists at that depth. */
int golhip_skew_interior_plan(golhip_t h, int32_t depth, int32_t ext, int32_t counts, int64_t *interior_bodies,
                              int64_t *main_bodies);

/* ---- board I/O -------------------------------------------------------- */
/* Load this handle's rows (height x width bytes, or its strip's rows). */
int golhip_load_bytes(golhip_t h, const uint8_t *cells);
/* The same rows as bit words (rows x ceil(width/32) uint32, cell (y, x) = bit
 * x % 32 of word x / 32 of row y).  Where width % 32 != 0 the bits of columns
 * >= width in the last word of a row are ignored: they are cleared on the
 * device after the copy, so no count, digest, list or snapshot sees them. */
int golhip_load_bits(golhip_t h, const uint32_t *words);
/* Synthetic board: cell (y, x) alive <=> (splitmix64(seed ^ (y*width + x)) & 3) == 0,
 * global coordinates (strips of one board agree). */
int golhip_fill_random(golhip_t h, uint64_t seed);

/* ---- the turn loop ---------------------------------------------------- */
/* Enqueue nturns turns (asynchronous).  want_flips != 0 keeps the flip list
 * of the LAST turn for golhip_flips (initializeAliveCells, :212-220). */
int golhip_step(golhip_t h, int64_t nturns, int32_t want_flips);
int golhip_sync(golhip_t h);
int golhip_turn(golhip_t h, int64_t *turns_done);

/* ---- side channels ---------------------------------------------------- */
/* Alive cells of this handle's rows at turn *at_turn (len(calculateAliveCells)). */
int golhip_alive_count(golhip_t h, uint64_t *count, int64_t *at_turn);
/* Sum over the RCCL ring (equals golhip_alive_count without a comm). */
int golhip_alive_count_global(golhip_t h, uint64_t *count, int64_t *at_turn);
/* Cells that changed in the last stepped turn (want_flips), row-major,
 * (x = col, y = row) pairs in global coordinates.  ERANGE sets *n.  The list
 * stays until the board is stepped, loaded, cleared or stamped: observers
 * (counts, snapshots, golhip_alive_cells, frames, checkpoints) keep it.
 * GOLHIP_EINVAL where the handle keeps no list of its current turn:
 * golhip_step_flips and the flip streams (a group's, and those of a handle or
 * a group with another rule than Conway's included) return their lists and
 * keep none. */
int golhip_flips(golhip_t h, int32_t *xy, uint64_t cap, uint64_t *n);
/* Batched CellFlipped stream (distributor.go:93-173 with the per-turn
 * initializeAliveCells :212-220): advance nturns turns one at a time and
 * return every turn's flip list, concatenated in turn order (row-major within
 * a turn, same pairs as golhip_flips), with counts[t] = flips of turn t.
 * One host round trip for the whole batch, on the fused turn + list kernel
 * (K5).  The board always advances nturns; if the lists exceed cap pairs, xy
 * holds the first cap, *n the total and the call returns GOLHIP_ERANGE.
 * Reserves min(cap, nturns x cells) pairs on the device.  Works in a
 * multi-rank ring; golhip_flip_stream (below) never drops a flip. */
int golhip_step_flips(golhip_t h, int64_t nturns, int32_t *xy, uint64_t cap, uint64_t *counts, uint64_t *n);
/* The CellFlipped stream without loss: advance UP TO nturns turns, one at a
 * time, each fused with its flip list on the device (initializeAliveCells,
 * :212-220), and append the lists in turn order to `out` (row-major within a
 * turn): format GOLHIP_FLIPS_XY = int32 (x = col, y = row) pairs, 8 bytes a
 * flip; GOLHIP_FLIPS_INDEX = uint32 y * width + x, 4 bytes a flip (boards of
 * at most 2^32 cells).  cap counts entries.  The batch stops before the
 * first turn whose list would not fit, so no flip is ever dropped: the board
 * is left at the last turn that fitted, *turns_done says how many ran
 * (counts[t] for t < *turns_done), *n = entries written.  If not even the
 * first turn fits: GOLHIP_ERANGE, nothing advanced, *n = entries it needs.
 * A batch may also stop short of a turn that would have fitted (it launches
 * the turns the last batch's largest list says the buffer holds); where it
 * does, a second call with the same buffer continues.  The first batch after
 * the board was replaced (a load, fill, clear, checkpoint or image load) runs
 * every turn that fits.
 * One host round trip per call.  Not for multi-rank rings (a stop on one
 * rank would desynchronise them): use golhip_step_flips there. */
#define GOLHIP_FLIPS_XY 0
#define GOLHIP_FLIPS_INDEX 1
int golhip_flip_stream(golhip_t h, int64_t nturns, int32_t format, void *out, uint64_t cap, uint64_t *counts,
                       int64_t *turns_done, uint64_t *n);
/* golhip_flip_stream of the whole board held by the group of row strips `hs`
 * (the group golhip_group_step takes; every strip at the same turn, else
 * GOLHIP_EINVAL): the same contract, word for word.  Up to nturns turns one at
 * a time; each turn's list is appended to `out` in turn order, row-major over
 * the whole torus within a turn (strip order), coordinates global; counts[t]
 * is the board's count of turn t; the batch stops before the first turn whose
 * board-wide list would not fit in cap entries and leaves EVERY strip at that
 * turn (golhip_group_step / golhip_step* continue from there); if not even the
 * first turn fits: GOLHIP_ERANGE, nothing advanced, *n_entries = what it
 * needs.  Every width: K5 per strip and turn into device
 * lists, no host synchronisation between turns, then one gather launch a
 * strip that writes `out` itself where it lies in golhip_host_alloc memory
 * mapped on the strip's device: two host round trips a call.  (Only strips of
 * 2^32 - 4096 words or more go one group turn at a time through the any-width
 * kernel, two round trips a turn.)  With n == 1 and a
 * whole-torus handle it is golhip_flip_stream.  In-process groups only (not
 * multi-rank rings). */
int golhip_group_flip_stream(golhip_t *hs, int32_t n, int64_t nturns, int32_t format, void *out, uint64_t cap,
                             uint64_t *counts, int64_t *turns_done, uint64_t *n_entries);
/* Alive cells, row-major (x = col, y = row) pairs — calculateAliveCells. */
int golhip_alive_cells(golhip_t h, int32_t *xy, uint64_t cap, uint64_t *n);
/* Board as 0/255 bytes / bit words (this handle's rows). */
int golhip_snapshot_bytes(golhip_t h, uint8_t *out);
int golhip_snapshot_bits(golhip_t h, uint32_t *out);
/* Bit words of rows [row, row + nrows) of this handle (nrows x ceil(width/32)
 * uint32): a few rows of a board too large to copy whole (the 262144^2
 * full-size checks). */
int golhip_snapshot_rows(golhip_t h, int32_t row, int32_t nrows, uint32_t *out);
/* Order-independent board digest: sum over words of
 * splitmix64((global_word_index << 32) | word) mod 2^64 (strips add up). */
int golhip_board_hash(golhip_t h, uint64_t *hash);

/* ---- live view -------------------------------------------------------- */
/* A frame of the board for a window (the reference's sdl/window.go): out_w x
 * out_h pixels, row-major, pixel (px, py) covering the s x s cells
 *   x in [x0 + px s, x0 + px s + s) mod width,
 *   y in [y0 + py s, y0 + py s + s) mod height.
 * With n alive cells in that block, g = (255 n + s^2 - 1) / s^2 in integers:
 * rounded up, so 0 only for an empty block (one glider shows at any scale)
 * and 255 for a full one.  GRAY8 stores g, ARGB8888 stores g * 0x01010101; at
 * s = 1 that is the pixel buffer of the reference's Window after its flips
 * (FF FF FF FF or zeros) and the number of 0xFFFFFFFF pixels is its
 * CountPixels().
 * Required: 0 <= x0 < width, 0 <= y0 < height, 1 <= scale <=
 * GOLHIP_VIEW_MAX_SCALE, out_w, out_h >= 1, out_w * scale <= width,
 * out_h * scale <= height: at most one lap, which may cross the seam in x and
 * in y.  On a strip handle y counts torus rows and [y0, y0 + out_h * scale)
 * must lie inside the strip's rows (x still wraps).  The frame is rendered on
 * the device from the board as it is stepped (no layout conversion, nothing
 * of the board is written) and costs the same whatever the activity. */
#define GOLHIP_VIEW_ARGB8888 0   /* uint32 per pixel, the SDL texture format of sdl/window.go:32 */
#define GOLHIP_VIEW_GRAY8 1      /* uint8 per pixel (PGM-ready) */
#define GOLHIP_VIEW_MAX_SCALE 1024
typedef struct golhip_view {
    int32_t x0, y0;        /* top-left cell of the viewport, torus coordinates */
    int32_t scale;         /* s >= 1: one pixel covers s x s cells */
    int32_t out_w, out_h;  /* frame size in pixels */
    int32_t format;        /* GOLHIP_VIEW_* */
} golhip_view_t;
/* The frame of the current board (synchronous; *at_turn, nullable, is the turn
 * it shows).  GOLHIP_ERANGE when cap_bytes is smaller than the frame.  If out
 * lies inside golhip_host_alloc memory the kernel writes it there itself. */
int golhip_view_frame(golhip_t h, const golhip_view_t *v, void *out, uint64_t cap_bytes, int64_t *at_turn);
/* golhip_step(h, nturns, 0) with a frame rendered behind every `every`-th turn
 * on the handle's stream (no host synchronisation between turns): out
 * receives floor(nturns / every) consecutive frames, *frames (nullable) their
 * number, *turns_done (nullable) the turns advanced (nturns; turns after the
 * last frame are stepped too).  GOLHIP_ERANGE, with nothing advanced, when the
 * frames exceed cap_frames.  Returns after the last frame has landed. */
int golhip_view_stream(golhip_t h, int64_t nturns, int64_t every, const golhip_view_t *v, void *out,
                       uint64_t cap_frames, uint64_t *frames, int64_t *turns_done);
/* The same frame of a board held as the n row strips hs (the group of
 * golhip_group_step: one board, strips contiguous from row 0 and covering it,
 * one word layout; all loaded and at the same turn, else GOLHIP_EINVAL).  v is
 * a view of the whole torus: any viewport of at most one lap, across strip
 * boundaries and both seams.  No strip's rows are copied: every strip renders
 * the pixel rows that lie wholly inside it on its own stream and device, and
 * for a pixel row that straddles strips each of them adds up its part of the
 * alive counts, which the first strip of the viewport sums and normalises.
 * With n == 1 and a whole-torus handle this is golhip_view_frame. */
int golhip_group_view_frame(golhip_t *hs, int32_t n, const golhip_view_t *v, void *out, uint64_t cap_bytes,
                            int64_t *at_turn);
/* golhip_group_step(hs, n, every) with a group frame enqueued behind it,
 * floor(nturns / every) times, with no host synchronisation between turns; then
 * the remaining turns, and one synchronisation of every strip's stream.
 * Results as golhip_view_stream (GOLHIP_ERANGE with nothing advanced). */
int golhip_group_view_stream(golhip_t *hs, int32_t n, int64_t nturns, int64_t every, const golhip_view_t *v, void *out,
                             uint64_t cap_frames, uint64_t *frames, int64_t *turns_done);

/* ---- checkpoint and resume -------------------------------------------- */
/* Fault tolerance as checkpoint and restart (the reference README's third
 * extension, and its "a new controller should be able to take over" after
 * `q`): a GPU fault or a pre-empted job ends the process, so the state that
 * survives is a file, and a new process resumes from it at its turn.
 *
 * The file, little-endian, exactly 64 + 4 * height * Ww bytes, Ww =
 * ceil(width / 32): eight uint64 -- the bytes "GOLCKPT" 0x01; version 1 | 64
 * << 32; width | height << 32; the turn; the board's alive cells; its
 * golhip_board_hash; Ww; and the sum over i = 0..6 of splitmix64(q_i + i) --
 * then the board's bit words as golhip_snapshot_bits gives them, row-major
 * over the whole torus.  It does not depend on the word layout, the strips or
 * the devices: one board at one turn gives one file.
 *
 * hs, n: one whole-torus handle (n = 1) or the group golhip_group_step takes
 * (strips contiguous from row 0, covering the board).  golhip_checkpoint_begin
 * is not for handles of an RCCL ring (GOLHIP_EINVAL, one-rank rings included).
 * golhip_checkpoint_load takes the handle of a one-rank ring as the whole torus
 * it is (the turns after it are planned as before the load) and
 * refuses a rank of a larger ring: it is no group (GOLHIP_EINVAL).
 *
 * The file does not record the rule (golhip_set_rule; format version 1
 * stays): golhip_checkpoint_load leaves the handles' rule as it is, and a
 * process that resumes a run on another rule than Conway's sets it again. */
typedef struct golhip_ckpt golhip_ckpt;
typedef struct golhip_ckpt_opts {
    int32_t chunk_rows;   /* rows a staging buffer holds; 0 = automatic (16 MiB)  */
    int32_t reserved[3];  /* zero                                                 */
} golhip_ckpt_opts_t;
typedef struct golhip_ckpt_info {
    int32_t width, height;
    int64_t turn;
    uint64_t alive, hash, file_bytes;
    double stall_ms;   /* device time of the checkpoint kernels (sum over strips; HIP events) */
    double drain_ms;   /* from the first copy to the last byte in the staging buffers          */
    double write_ms;   /* from opening <path>.tmp to the rename                               */
} golhip_ckpt_info_t;
/* Starts a checkpoint of the board at its current turn (every strip at the
 * same turn, else GOLHIP_EINVAL) and returns once it is enqueued, without
 * synchronising the host.  Each handle's stream gets one kernel behind the
 * turns already enqueued: it reads the rows in the layout they are stepped in,
 * writes nothing to them, and stores the canonical words, their count and
 * their digest to a shadow buffer that the checkpoint object owns.  Turns
 * enqueued afterwards run on at once.  Behind the kernel a side stream of the
 * object copies the shadow to the host in chunks of chunk_rows rows through
 * two page-locked buffers, and a writer thread writes each chunk at its place
 * in <path>.tmp, then the header, then fsyncs and renames it over <path>: an
 * existing <path> stays whole until that moment, whatever fails.  A handle's
 * mutex is held for its own enqueue only.  A second begin on a handle first
 * waits until the earlier checkpoint of that handle has left the device (it
 * neither joins nor frees it).  golhip_destroy of the handles is legal as soon
 * as begin has returned.  opts nullable. */
int golhip_checkpoint_begin(golhip_t *hs, int32_t n, const char *path, const golhip_ckpt_opts_t *opts,
                            golhip_ckpt **out);
/* Joins the writer, reports (info nullable) and frees ck.  File errors
 * (GOLHIP_EINVAL: <path>.tmp cannot be created, written or renamed) and device
 * errors are reported here; no <path>.tmp is left behind either outcome. */
int golhip_checkpoint_wait(golhip_ckpt *ck, golhip_ckpt_info_t *info);
/* Header and size of a checkpoint file (timings zero); needs no device.
 * GOLHIP_ECORRUPT, the message naming the check, for a wrong magic, version,
 * header check or file size; GOLHIP_EINVAL if it cannot be opened. */
int golhip_checkpoint_info(const char *path, golhip_ckpt_info_t *info);
/* Fills each handle's rows [row0, row0 + rows) from the file, chunk by chunk
 * through page-locked buffers (the file is never held whole), in the layout
 * the handle steps in, and sets every handle's turn to the file's: the one way
 * to a turn other than 0.  Counts and flip lists kept by the handles are
 * dropped as golhip_load_bits drops them.  The kernel that stores the rows
 * clears the bits of columns >= width and sums count and digest of what it
 * stored; the strips' sums must equal the header's.  A file of another width
 * or height: GOLHIP_EINVAL.  A bad magic, version, header check, file size,
 * count or digest: GOLHIP_ECORRUPT, the message naming the check.  After an
 * error the handles' boards are unspecified.  opts, info nullable. */
int golhip_checkpoint_load(golhip_t *hs, int32_t n, const char *path, const golhip_ckpt_opts_t *opts,
                           golhip_ckpt_info_t *info);

/* ---- PGM images, streamed ---------------------------------------------- */
/* The board as the reference's image file (gol/io.go:42-126): "P5\n" W " " H
 * "\n255\n", then height * width bytes, row-major, 255 alive and 0 dead --
 * byte for byte what writePgmImage writes.  It does not depend on the word
 * layout, the strips or the devices: one board at one turn gives one file.
 * Written behind the following turns as a checkpoint is, read chunk by chunk:
 * neither side ever holds width * height bytes on the host.
 *
 * hs, n: as for checkpoints.  golhip_image_begin refuses handles of an RCCL
 * ring (GOLHIP_EINVAL). */
typedef struct golhip_image golhip_image;
typedef struct golhip_image_info {
    int32_t width, height;
    int64_t turn;          /* begin: the turn the image shows; load/info: 0 */
    uint64_t alive;        /* begin, load: alive cells of the image         */
    uint64_t file_bytes;   /* header + width * height                       */
    uint32_t header_bytes, reserved;
    double stall_ms, drain_ms, write_ms;   /* as golhip_ckpt_info_t */
} golhip_image_info_t;
/* golhip_checkpoint_begin's contract with another format: returns once
 * enqueued, without synchronising the host.  Each handle's stream gets the
 * checkpoint's kernel (canonical words and the alive count to a shadow the
 * object owns); turns enqueued afterwards run on at once.  On the device's
 * side stream, behind that kernel, one expand kernel a chunk of chunk_rows
 * rows (0: the rows that fit 16 MiB of raster, at least one) writes the
 * chunk's bytes straight into one of two page-locked buffers, and a writer
 * thread writes each chunk at its place in <path>.tmp, then the header, then
 * fsyncs and renames it over <path>: an existing <path> stays whole until that
 * moment, and no <path>.tmp is left whatever fails.  A second begin on a
 * handle (image or checkpoint: they share the slot) first waits until the
 * earlier one has left the device.  golhip_destroy of the handles is legal as
 * soon as begin has returned.  opts nullable. */
int golhip_image_begin(golhip_t *hs, int32_t n, const char *path, const golhip_ckpt_opts_t *opts, golhip_image **out);
/* Joins the writer, reports (info nullable) and frees im.  File errors
 * (GOLHIP_EINVAL) and device errors are reported here. */
int golhip_image_wait(golhip_image *im, golhip_image_info_t *info);
/* The header of an image file, parsed as readPgmImage parses it (four
 * whitespace-separated fields, the raster one byte behind the fourth; bytes
 * behind the raster are ignored); needs no device.  GOLHIP_EINVAL with the
 * reference's message, checked in this order: "open <path>: no such file or
 * directory", "Not a pgm file", "Incorrect width" / "Incorrect height" (no
 * board to compare with here: a size outside 1 .. 2^31 - 1), "Incorrect
 * maxval/bit depth", "short raster in <path>". */
int golhip_image_info(const char *path, golhip_image_info_t *info);
/* The same checks, with "Incorrect width" / "Incorrect height" (behind the
 * magic) for a board other than the handles'; then each handle's rows are read
 * through two page-locked buffers in chunks of chunk_rows rows, chunk k + 1
 * from the file while chunk k is copied and packed (alive <=> byte 255), and
 * the load ends as golhip_load_bytes ends: turn 0, count and flip list
 * dropped.  info->alive is the handles' count after the load.  After an error
 * the handles' boards are unspecified.  opts, info nullable. */
int golhip_image_load(golhip_t *hs, int32_t n, const char *path, const golhip_ckpt_opts_t *opts,
                      golhip_image_info_t *info);
/* Waits until the last checkpoint or image begun on each of these handles has
 * left the device (its shadow drained to the staging buffers; its file may
 * still be written): what a following golhip_checkpoint_begin or
 * golhip_image_begin would otherwise wait for inside the call.  A caller that
 * begins under a lock of its own waits here first, outside it.  Returns at
 * once where nothing is in flight. */
int golhip_drain_wait(golhip_t *hs, int32_t n);
/* Test hook (GOLHIP_TEST_HOOKS=1): the expand kernel alone.  words: nrows *
 * ceil(width / 32) canonical words; the raster of rows [row0, row0 + nr) goes
 * to out[0, nr * width), and out[nr * width, out_bytes) must come back as the
 * caller filled it (the kernel writes into a page-locked copy of `out`). */
int golhip_test_image_expand(int32_t device, const uint32_t *words, int32_t width, int32_t nrows, int32_t row0,
                             int32_t nr, uint8_t *out, uint64_t out_bytes);

/* ---- patterns ----------------------------------------------------------- */
/* An empty board, and a rectangle of cells stamped anywhere on the torus: the
 * way to put a prepared pattern (a glider gun, a fleet, an experiment) on a
 * board too large to load as an image.  The stamp runs on the device, in the
 * layout the board is stepped in, at turn 0 or mid-run; results never depend
 * on the words per lane, the padded torus, the strip count or the launch plan.
 *
 * golhip_clear: every cell of this handle's rows dead; it ends as
 * golhip_load_bits ends: turn 0, count and flip list dropped.
 *
 * golhip_stamp_bits: `words` is a pattern of pw x ph cells as bit words, ph
 * rows of ceil(pw / 32) uint32 (cell (r, c) = bit c % 32 of word c / 32 of row
 * r; the bits of columns >= pw in a row's last word are ignored).  Its
 * top-left corner goes to the torus cell (x0, y0): pattern cell (r, c) meets
 * board cell ((y0 + r) mod height, (x0 + c) mod width).  Inside that rectangle
 *   GOLHIP_STAMP_COPY   the board becomes the pattern, dead cells included;
 *   GOLHIP_STAMP_OR     cells alive in the pattern come alive;
 *   GOLHIP_STAMP_XOR    cells alive in the pattern flip;
 *   GOLHIP_STAMP_CLEAR  cells alive in the pattern die;
 * cells outside it are never written.  Required: 0 <= x0 < width, 0 <= y0 <
 * height, 1 <= pw <= width, 1 <= ph <= height (at most one lap, which may
 * cross both seams); anything else is GOLHIP_EINVAL, and so are an unknown op,
 * a null pointer and a board never loaded: the board is then unchanged.
 * The turn does not change: a stamp edits the board at the turn it is at.  The
 * alive count and the flip list the handle keeps are dropped as a load drops
 * them (the next golhip_alive_count recounts).  The call stages the words in
 * device scratch (the buffer is not retained), runs behind whatever is
 * enqueued on the handle's stream (a checkpoint or image begun earlier shows
 * the board as it was before the stamp) and synchronises the stream before it
 * returns.  On a strip handle y counts torus rows, and pattern rows that fall
 * on rows the strip does not own are skipped (halo rows are not written: every
 * step exchanges them before its first launch; a rank of a ring is a strip
 * like any other).  golhip_group_stamp_bits stamps the board held by the group
 * of row strips golhip_group_step takes: every strip takes its rows. */
#define GOLHIP_STAMP_COPY 0
#define GOLHIP_STAMP_OR 1
#define GOLHIP_STAMP_XOR 2
#define GOLHIP_STAMP_CLEAR 3
int golhip_clear(golhip_t h);
int golhip_stamp_bits(golhip_t h, const uint32_t *words, int32_t pw, int32_t ph, int32_t x0, int32_t y0, int32_t op);
int golhip_group_stamp_bits(golhip_t *hs, int32_t n, const uint32_t *words, int32_t pw, int32_t ph,
                            int32_t x0, int32_t y0, int32_t op);
/* Pattern files, told apart by their first bytes, not their names: a PGM
 * image ("P5", alive <=> byte 255, the checks and messages of
 * golhip_image_info) or else RLE, the run-length format Life programs
 * exchange: '#' lines, the header "x = m, y = n[, rule = r]", then runs
 * <count><b|o|$> ended by '!', white space anywhere between the body's
 * characters, trailing dead cells and rows optional.  Only Conway's rule is
 * read: B3/S23 (either case), 23/3, or none.  GOLHIP_EINVAL with a message
 * naming the check: no header, another rule, a size outside 1 .. 2^31 - 1, a
 * run that leaves the x by y box, an unknown character, no '!' before the end
 * of the file (and a file that cannot be opened). */
typedef struct golhip_pattern_info {
    int32_t width, height;
    uint64_t alive;
    int32_t format;        /* 0 RLE, 1 PGM */
    int32_t reserved;
} golhip_pattern_info_t;
/* Size, alive cells and format of a pattern file: the whole body is parsed in
 * one pass and nothing of the size of width * height is allocated.  Needs no
 * device. */
int golhip_pattern_info(const char *path, golhip_pattern_info_t *info);
/* The pattern as golhip_stamp_bits takes it: height * ceil(width / 32) words
 * (padding bits zero).  GOLHIP_ERANGE when cap_words is smaller, with
 * info->width and height set (alive 0): the size is checked before anything is
 * written.  Needs no device. */
int golhip_pattern_read(const char *path, uint32_t *words, uint64_t cap_words, golhip_pattern_info_t *info);
/* The rule an RLE file's header names, as golhip_rule_parse's masks; Conway's
 * where it names none or the file is a PGM.  GOLHIP_EINVAL for a rule
 * golhip_rule_parse refuses and for the file errors of golhip_pattern_info
 * (which, like golhip_pattern_read, goes on refusing every rule but
 * Conway's).  Needs no device. */
int golhip_pattern_rule(const char *path, uint32_t *birth, uint32_t *survive);
/* golhip_pattern_read and golhip_group_stamp_bits in one call (hs, n: one
 * whole-torus handle or a group of strips).  A pattern larger than the board
 * is refused before its cells are read.  info nullable.
 * On handles with Conway's rule the file's rule is checked as by
 * golhip_pattern_info; on handles whose rule is R (golhip_set_rule) an RLE
 * file must name R (any spelling golhip_rule_parse takes) or no rule at all:
 * any other is GOLHIP_EINVAL with a message naming both rules. */
int golhip_stamp_file(golhip_t *hs, int32_t n, const char *path, int32_t x0, int32_t y0, int32_t op,
                      golhip_pattern_info_t *info);

/* ---- saving patterns ---------------------------------------------------- */
/* The way back: any rectangle of the torus as bit words, the smallest box
 * around the alive cells, and an RLE file of either.  The
 * extract (K12) and the occupancy pass (K13) read the board on the device in
 * the layout it is stepped in and never write it; results never depend on the
 * words per lane, the strip count or the launch plan.
 *
 * golhip_extract_bits: the pw x ph cells whose top-left corner is the torus
 * cell (x0, y0), as golhip_stamp_bits takes them: ph rows of ceil(pw / 32)
 * uint32, pattern cell (r, c) = board cell ((y0 + r) mod height, (x0 + c) mod
 * width), padding bits zero.  The requirements are the stamp's: 0 <= x0 <
 * width, 0 <= y0 < height, 1 <= pw <= width, 1 <= ph <= height, a board
 * loaded, no null pointer (GOLHIP_EINVAL); cap_words < ph * ceil(pw / 32) is
 * GOLHIP_ERANGE.  On a strip handle y counts torus rows and the rows the strip
 * does not own come back zero, as the stamp skips them (a rank of a ring is a
 * strip like any other).  golhip_group_extract_bits reads the board held by
 * the group of row strips golhip_group_step takes: every row of the rectangle
 * comes from the strip that owns it.
 *
 * golhip_alive_box (hs, n: one whole-torus handle or a group of strips): the
 * smallest box of at most one lap that holds every alive cell of the torus,
 * seams included: a glider that has walked across both seams has a 3 x 3 box
 * at (width - 1, height - 1).  Each side is golhip_box_interval of that axis'
 * occupancy.  *pw = *ph = 0 (and *x0 = *y0 = 0) on an empty board.
 *
 * All three are observers: the board, the turn, the kept count and the kept
 * flip list stay; they run behind whatever is enqueued on the handles' streams
 * and synchronise them.
 *
 * golhip_box_interval (no device; exposed for tests): `bits` is the occupancy
 * bitmap of a cyclic axis of n >= 1 positions (position p = bit p % 32 of word
 * p / 32).  (*start, *len) is the shortest cyclic interval that covers every
 * set bit, the complement of the longest cyclic run of clear bits; where
 * several runs tie for longest, the interval with the smallest start.  No set
 * bit: (0, 0).  No clear bit: (0, n). */
int golhip_extract_bits(golhip_t h, int32_t x0, int32_t y0, int32_t pw, int32_t ph, uint32_t *words,
                        uint64_t cap_words);
int golhip_group_extract_bits(golhip_t *hs, int32_t n, int32_t x0, int32_t y0, int32_t pw, int32_t ph,
                              uint32_t *words, uint64_t cap_words);
int golhip_alive_box(golhip_t *hs, int32_t n, int32_t *x0, int32_t *y0, int32_t *pw, int32_t *ph);
int golhip_box_interval(const uint32_t *bits, int32_t n, int32_t *start, int32_t *len);
/* words as golhip_stamp_bits takes them -> an RLE file (no device): the line
 * "#CXRLE Pos=<x0>,<y0> Gen=<turn>" (Golly's extended header; golhip_pattern_*
 * skip '#' lines), "x = <pw>, y = <ph>, rule = <golhip_rule_format's
 * spelling>", then the body in lines of at most 70 characters, counts of 1,
 * trailing dead cells of a row and trailing dead rows left out, '!' at the
 * end.  A pattern with no alive cell is the header and "!".  The file is
 * written as <path>.tmp, fsynced and renamed over <path>; after a failure
 * (GOLHIP_EINVAL, the message names the call that failed) no .tmp is left. */
int golhip_pattern_write(const char *path, const uint32_t *words, int32_t pw, int32_t ph, uint32_t birth,
                         uint32_t survive, int32_t x0, int32_t y0, int64_t turn);
/* Box, extract and write in one call (hs, n: one whole-torus handle or a
 * group of strips), chunk_rows rows at a time (0: the rows that fit 16 MiB of
 * words, at least one): never more than one chunk is held on the host.  pw ==
 * 0 && ph == 0: the alive box (x0, y0 ignored); an empty board is then
 * GOLHIP_EINVAL "board is empty" and no file is written.  The header's rule
 * is the handles' rule, Pos the box's corner, Gen the handles' turn.  info
 * (nullable): width, height, alive as the writer counted them, format 0.  The
 * file is committed as golhip_pattern_write commits it. */
int golhip_save_rle(golhip_t *hs, int32_t n, const char *path, int32_t x0, int32_t y0, int32_t pw, int32_t ph,
                    int32_t chunk_rows, golhip_pattern_info_t *info);

/* ---- measurement ------------------------------------------------------ */
int golhip_perf(golhip_t h, golhip_perf_t *out);
/* Diagnostics of the persistent step kernels since the last call (option
 * "trace" must be set before stepping): out[0] = sum over waves of band
 * compute time, out[1] = longest band of one super-step, out[2] = sum over
 * workgroups of time spent waiting for neighbour workgroups, out[3] = sum
 * over workgroups of kernel time, out[4] = workgroup count; times in
 * s_memrealtime ticks (100 MHz).  No reference counterpart (measurement). */
int golhip_persist_trace(golhip_t h, uint64_t out[5]);
/* Per-wave (start, end) ticks of the middle super-step of the last persistent
 * launch: out[2 * (workgroup * 64 + wave) + {0, 1}], n words. */
int golhip_persist_trace_waves(golhip_t h, uint64_t *out, int64_t n);
int golhip_perf_reset(golhip_t h);

#ifdef __cplusplus
}
#endif
#endif /* GOLHIP_H */
