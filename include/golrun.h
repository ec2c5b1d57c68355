/*
 * golrun.h — C-ABI of libgolhost.so, the host-side mirror of the reference's
 * gol.Run (gol/gol.go:12) built on libgolhip.so.
 *
 * golrun_start is `go gol.Run(p, events, keyPresses)` (gol_test.go:34,
 * count_test.go:26): it starts the run on its own thread; golrun_next_event is
 * one receive of `for event := range events` (it returns 0 once the channel is
 * closed and drained); golrun_send_key is `keyPresses <- k`.
 * Event kinds, fields and String() text follow gol/event.go:19-131.
 */
#ifndef GOLRUN_H
#define GOLRUN_H

#include <stdint.h>

#include "golhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* golrun_start flags */
#define GOLRUN_FLAG_KEYS 0x1u            /* create a keyPresses channel (else nil)          */
#define GOLRUN_FLAG_REF_QUIRKS 0x2u      /* reference quirks: 0-based TurnComplete, transposed
                                            CellFlipped and s/q snapshots (DESIGN.md "Quirks") */
#define GOLRUN_FLAG_NO_CELL_EVENTS 0x4u  /* no per-cell CellFlipped (fused turns, fast)     */
#define GOLRUN_FLAG_NO_TURN_EVENTS 0x8u  /* no per-turn TurnComplete                        */
#define GOLRUN_FLAG_VIEW_STRIPS 0x10u    /* golrun_start_view: a run on row strips renders its
                                            view across them (golhip_group_view_frame)      */
/* Bit 5, 0x20u: beside the final image and the images of `s` and `q` the run
 * writes out/<W>x<H>x<turn>.rle, the alive box of the board at that turn
 * (golhip_save_rle; one handle or strips), complete before that image's
 * ImageOutputComplete; never transposed; an empty board writes no file and
 * prints a line saying so; image_every images get none (gol_host.h
 * RunOptions::save_rle; the environment's GOL_SAVE_RLE=1 does the same).
 * golrun_opts_t has no free slot left, hence a flag bit. */
#define GOLRUN_FLAG_SAVE_RLE (1u << 5)
/* Bit 6, 0x40u: a run with another rule than Conway's takes its CellFlipped
 * batches from the fused turn + list kernel (golhip_set_rule_flips 1 on every
 * handle, right after the rule); the events are the same either way (gol_host.h
 * RunOptions::rule_flips; the environment's GOL_RULE_FLIPS=1 does the same). */
#define GOLRUN_FLAG_RULE_FLIPS (1u << 6)
/* Bit 7, 0x80u: the run's board is a bounded plane, every cell outside it dead
 * for ever (golhip_set_topology GOLHIP_TOPOLOGY_PLANE on every handle, strips
 * included, right after the rule); the events are unchanged in kind (gol_host.h
 * RunOptions::plane; the environment's GOL_PLANE=1 does the same). */
#define GOLRUN_FLAG_PLANE (1u << 7)

/* event kinds (gol/event.go) */
#define GOLRUN_ALIVE_CELLS_COUNT 0
#define GOLRUN_IMAGE_OUTPUT_COMPLETE 1
#define GOLRUN_STATE_CHANGE 2
#define GOLRUN_CELL_FLIPPED 3
#define GOLRUN_TURN_COMPLETE 4
#define GOLRUN_FINAL_TURN_COMPLETE 5
/* State (event.go:33-38) */
#define GOLRUN_PAUSED 0
#define GOLRUN_EXECUTING 1
#define GOLRUN_QUITTING 2

typedef struct golrun golrun;
typedef golrun *golrun_t;

/* Go's int is 64-bit (event.go:19-68, util/cell.go:4-6): so are these. */
typedef struct golrun_event {
    int32_t kind;
    int32_t new_state;         /* StateChange.NewState                     */
    int64_t completed_turns;   /* GetCompletedTurns()                      */
    int64_t cells_count;       /* AliveCellsCount.CellsCount               */
    int64_t cell_x, cell_y;    /* CellFlipped.Cell                         */
    int64_t alive_len;         /* len(FinalTurnComplete.Alive)             */
    char filename[256];        /* ImageOutputComplete.Filename             */
    char text[288];            /* String()                                 */
} golrun_event_t;

const char *golrun_last_error(void);
/* root: directory with images/<W>x<H>.pgm; output goes to root/out/.
 * events_cap: 0 = unbuffered (as in the tests), 1000 as in main.go:53.
 * ticker_ms: AliveCellsCount period (<= 0: 2000 as distributor.go:285). */
int golrun_start(int64_t turns, int64_t threads, int64_t width, int64_t height, const char *root, int32_t device,
                 uint32_t flags, int32_t events_cap, int32_t ticker_ms, golrun_t *out);
/* golrun_start with a live view (the reference's SDL window as pixels): the
 * run renders `view` (golhip.h, golhip_view_frame's pixels) on the device
 * after every `every`-th turn (>= 1) and publishes the frame before that
 * turn's TurnComplete is sent; the frame of turn 0 is there before the first
 * event, the final board's before FinalTurnComplete.  With cell events on,
 * frames are rendered between the flip-stream batches instead (each shows its
 * batch's last turn).  Runs of more than one strip (GOL_STRIPS / GOL_NGPU)
 * are refused (golrun_wait reports the message) unless GOLRUN_FLAG_VIEW_STRIPS
 * or the environment's GOL_VIEW_STRIPS=1 opts in: then the frames are
 * golhip_group_view_frame's, the same pixels. */
int golrun_start_view(int64_t turns, int64_t threads, int64_t width, int64_t height, const char *root,
                      int32_t device, uint32_t flags, int32_t events_cap, int32_t ticker_ms,
                      const golhip_view_t *view, int32_t every, golrun_t *out);
/* golrun_start_view with checkpointing and resume (gol_host.h RunOptions):
 * view nullable (view_every is then ignored).
 * checkpoint_path (nullable): a checkpoint file (golhip.h) is written there at
 * every turn that is a multiple of checkpoint_every (0: none) behind the
 * following turns, the last one before FinalTurnComplete; on `q` one of the
 * turn the run stops at, complete before StateChange{Quitting}: the state a
 * new controller takes over.
 * resume_path (nullable): board and turn T come from that checkpoint instead
 * of images/<W>x<H>.pgm.  Its size must equal width x height and T <= turns,
 * else the run fails where the image read fails (golrun_wait has the message,
 * no event is sent).  The initial CellFlipped events are the alive cells of
 * that board at turn T; TurnComplete continues at T + 1; T == turns goes
 * straight to FinalTurnComplete.
 * reserved[1]: stream_images (gol_host.h RunOptions::stream_images): 1 puts the
 * images/ and out/ files through golhip_image_* (the load in chunks; the s, q
 * and final images written behind the turns), 0 leaves it to the environment's
 * GOL_STREAM_IMAGES=1.  golrun_start has no flag bit for it.
 * reserved[0]: image_every (gol_host.h RunOptions::image_every; 0: none): with
 * streamed images, out/<W>x<H>x<turn>.pgm at every turn that is a multiple of
 * it, behind the following turns, each with its ImageOutputComplete once the
 * file is complete.  Without streamed images the run fails with a message.
 * reserved[2]: patterns (gol_host.h RunOptions::patterns; 0: none): a pointer
 * (cast to int64_t) to a NUL-terminated string with one "path@x,y[,op]" a
 * line, op one of copy|or|xor|clear (default or): pattern files (RLE or PGM,
 * golhip_stamp_file) stamped in that order, top-left corner at the torus cell
 * (x, y), after the initial board is there and before any event; the initial
 * CellFlipped events are the alive cells of the board after the stamps.  The
 * string is copied before golrun_start_opts returns; a spec that does not
 * parse fails the call itself (golrun_last_error), an unreadable file or a
 * pattern that does not fit fails the run where the image read fails.
 * reserved[3]: blank (RunOptions::blank): 1 starts from an empty board
 * (golhip_clear) instead of images/<W>x<H>.pgm.
 * With resume_path, patterns and blank are refused where the image read
 * fails: a restarted job must not stamp twice.
 * reserved0: the run's Life-like rule (gol_host.h RunOptions::rule): 0 is
 * Conway's B3/S23, any other rule is 0x40000 | survive << 9 | birth with the
 * 9-bit masks of golhip_rule_parse (bit 18 tells B/S with both masks empty
 * from 0; any other bit set fails the call).  The rule is set on every handle
 * of the run, strips included, before the initial board's events.  With
 * resume_path the caller passes the rule again: a checkpoint keeps none.
 * Pattern files must name the run's rule or none (golhip_stamp_file). */
typedef struct golrun_opts {
    const golhip_view_t *view;
    int32_t view_every;
    int32_t reserved0;      /* the rule: 0 Conway, else 0x40000 | survive << 9 | birth */
    const char *checkpoint_path;
    int64_t checkpoint_every;
    const char *resume_path;
    int64_t reserved[4];    /* [0]: image_every; [1]: stream_images; [2]: patterns; [3]: blank */
} golrun_opts_t;
int golrun_start_opts(int64_t turns, int64_t threads, int64_t width, int64_t height, const char *root,
                      int32_t device, uint32_t flags, int32_t events_cap, int32_t ticker_ms,
                      const golrun_opts_t *opts, golrun_t *out);
/* Copy of the newest published frame and the turn its pixels show.  After
 * TurnComplete{t} of a run with every = 1 that turn is >= t; while paused it
 * stays at the paused turn; after FinalTurnComplete it is the final board.
 * GOLHIP_ERANGE when cap_bytes is smaller than the frame, GOLHIP_EINVAL when
 * the run has no view or nothing is published yet. */
int golrun_view_frame(golrun_t r, void *out, uint64_t cap_bytes, int64_t *turn);
/* 1 = event received, 0 = channel closed and drained, 2 = timeout (timeout_ms >= 0). */
int golrun_next_event(golrun_t r, golrun_event_t *ev, int32_t timeout_ms);
/* Alive list of the last FinalTurnComplete received (alive_len pairs X, Y). */
int golrun_event_cells(golrun_t r, int64_t *xy, uint64_t cap);
/* String() of an event's fields (event.go:72-131); needs no run or device. */
int golrun_event_string(const golrun_event_t *ev, char *out, uint64_t cap);
/* main.go's headless drain loop (main.go:59-66) on the run's own events, for
 * runs whose event streams are too large to hand over one by one: receives
 * until the channel closes and tallies count[kind].  For CellFlipped of
 * completed turn t in 1..turns_cap (documented contract: 1-based turns):
 * flips[t-1] events and digests[t-1] = sum over them, in arrival order, of
 * splitmix64(i) * (Y * width + X + 1), i = 1, 2, ... within the turn
 * (tests/golden/make_fullsize.py ordered_digest).  flips / digests nullable. */
typedef struct golrun_drain_stats {
    uint64_t count[6];     /* events received, by GOLRUN_* kind              */
    int64_t last_turn;     /* CompletedTurns of the last TurnComplete        */
    int64_t final_alive;   /* len(FinalTurnComplete.Alive), 0 if none         */
} golrun_drain_stats_t;
int golrun_drain(golrun_t r, golrun_drain_stats_t *st, uint64_t *flips, uint64_t *digests, int64_t turns_cap,
                 int64_t width);
int golrun_send_key(golrun_t r, uint32_t key);
/* Drains unread events, joins the run; 0 or the panic message in err. */
int golrun_wait(golrun_t r, char *err, uint64_t err_cap);
int golrun_destroy(golrun_t r);

#ifdef __cplusplus
}
#endif
#endif /* GOLRUN_H */
