package gol

// The cgo binding of libgolhip.so (include/golhip.h), the MI355X engine that
// replaces the reference's turn loop (gol/distributor.go:93-173) and its side
// channels.  Dropped into the reference's gol package together with
// distributor.go from this directory (INTEGRATION.md); this repository is
// expected at ../engine, next to the reference's gol/ directory, with
// libgolhip.so built (make -C engine/game-of-life-distributed_amd/csrc).
//
// Go memory handed to C (the loaded board, the count slices) is only used
// during the call (cgo pointer rules); the flip buffer is C memory
// (golhip_host_alloc: page-locked, written by the device directly).

// #cgo CFLAGS: -I${SRCDIR}/../engine/include
// #cgo LDFLAGS: -L${SRCDIR}/../engine/game-of-life-distributed_amd/golhip -lgolhip -Wl,-rpath,${SRCDIR}/../engine/game-of-life-distributed_amd/golhip
// #include <stdio.h>
// #include <stdlib.h>
// #include "golhip.h"
//
// // golhip_last_error() is thread-local and a goroutine may move to another OS
// // thread between two cgo calls, so every checked call returns its status
// // together with the message, read in the same C call (same thread).
// typedef struct { int rc; char msg[320]; } gh_status;
// static gh_status gh_wrap(int rc) {
//     gh_status s;
//     s.rc = rc;
//     s.msg[0] = 0;
//     if (rc != GOLHIP_OK) snprintf(s.msg, sizeof s.msg, "%s", golhip_last_error());
//     return s;
// }
// static gh_status gh_create(int32_t w, int32_t h, golhip_t *out) { return gh_wrap(golhip_create(w, h, 0, 0, out)); }
// static gh_status gh_create_strip(int32_t w, int32_t h, int32_t r0, int32_t rows, int32_t dev, golhip_t *out) {
//     return gh_wrap(golhip_create_strip(w, h, r0, rows, dev, 0, out));
// }
// static gh_status gh_device_count(int32_t *n) { return gh_wrap(golhip_device_count(n)); }
// static gh_status gh_load_bytes(golhip_t h, const uint8_t *c) { return gh_wrap(golhip_load_bytes(h, c)); }
// static gh_status gh_host_alloc(uint64_t b, void **p) { return gh_wrap(golhip_host_alloc(b, p)); }
// static gh_status gh_group_step_ex(golhip_t *hs, int32_t n, int64_t t, int32_t f) {
//     return gh_wrap(golhip_group_step_ex(hs, n, t, f));
// }
// static gh_status gh_step_sync(golhip_t h, int64_t t) {
//     int rc = golhip_step(h, t, 0);
//     return gh_wrap(rc != GOLHIP_OK ? rc : golhip_sync(h));
// }
// static gh_status gh_flip_stream(golhip_t h, int64_t t, void *out, uint64_t cap, uint64_t *counts, int64_t *done,
//                                 uint64_t *n) {
//     return gh_wrap(golhip_flip_stream(h, t, GOLHIP_FLIPS_INDEX, out, cap, counts, done, n));
// }
// static gh_status gh_group_flip_stream(golhip_t *hs, int32_t n, int64_t t, void *out, uint64_t cap, uint64_t *counts,
//                                       int64_t *done, uint64_t *total) {
//     return gh_wrap(golhip_group_flip_stream(hs, n, t, GOLHIP_FLIPS_INDEX, out, cap, counts, done, total));
// }
// static gh_status gh_alive_cells(golhip_t h, int32_t *xy, uint64_t cap, uint64_t *n) {
//     return gh_wrap(golhip_alive_cells(h, xy, cap, n));
// }
// static gh_status gh_alive_count(golhip_t h, uint64_t *n, int64_t *t) { return gh_wrap(golhip_alive_count(h, n, t)); }
// static gh_status gh_snapshot_bytes(golhip_t h, uint8_t *out) { return gh_wrap(golhip_snapshot_bytes(h, out)); }
// static gh_status gh_view_frame(golhip_t h, const golhip_view_t *v, void *out, uint64_t cap, int64_t *turn) {
//     return gh_wrap(golhip_view_frame(h, v, out, cap, turn));
// }
// static gh_status gh_view_stream(golhip_t h, int64_t t, int64_t every, const golhip_view_t *v, void *out, uint64_t cap,
//                                 uint64_t *frames, int64_t *done) {
//     return gh_wrap(golhip_view_stream(h, t, every, v, out, cap, frames, done));
// }
// static gh_status gh_group_view_frame(golhip_t *hs, int32_t n, const golhip_view_t *v, void *out, uint64_t cap,
//                                      int64_t *turn) {
//     return gh_wrap(golhip_group_view_frame(hs, n, v, out, cap, turn));
// }
// static gh_status gh_group_view_stream(golhip_t *hs, int32_t n, int64_t t, int64_t every, const golhip_view_t *v,
//                                       void *out, uint64_t cap, uint64_t *frames, int64_t *done) {
//     return gh_wrap(golhip_group_view_stream(hs, n, t, every, v, out, cap, frames, done));
// }
// static gh_status gh_checkpoint_begin(golhip_t *hs, int32_t n, const char *path, golhip_ckpt **out) {
//     return gh_wrap(golhip_checkpoint_begin(hs, n, path, NULL, out));
// }
// static gh_status gh_checkpoint_wait(golhip_ckpt *ck) { return gh_wrap(golhip_checkpoint_wait(ck, NULL)); }
// static gh_status gh_checkpoint_info(const char *path, golhip_ckpt_info_t *info) {
//     return gh_wrap(golhip_checkpoint_info(path, info));
// }
// static gh_status gh_checkpoint_load(golhip_t *hs, int32_t n, const char *path) {
//     return gh_wrap(golhip_checkpoint_load(hs, n, path, NULL, NULL));
// }
// // Streamed PGM images (golhip_image_*; GOL_STREAM_IMAGES=1): the image of the
// // board at its current turn, written behind the following turns, and the
// // chunked load of images/<W>x<H>.pgm.
// static gh_status gh_image_begin(golhip_t *hs, int32_t n, const char *path, golhip_image **out) {
//     return gh_wrap(golhip_image_begin(hs, n, path, NULL, out));
// }
// static gh_status gh_image_wait(golhip_image *im) { return gh_wrap(golhip_image_wait(im, NULL)); }
// static gh_status gh_image_info(const char *path, golhip_image_info_t *info) {
//     return gh_wrap(golhip_image_info(path, info));
// }
// static gh_status gh_image_load(golhip_t *hs, int32_t n, const char *path) {
//     return gh_wrap(golhip_image_load(hs, n, path, NULL, NULL));
// }
// // Patterns (golhip_clear, golhip_stamp_bits, golhip_stamp_file): an empty
// // board, and a rectangle of cells stamped anywhere on the torus at the turn the
// // board is at; the group calls take one whole-torus handle as well.
// static gh_status gh_clear(golhip_t h) { return gh_wrap(golhip_clear(h)); }
// static gh_status gh_group_stamp_bits(golhip_t *hs, int32_t n, const uint32_t *words, int32_t pw, int32_t ph,
//                                      int32_t x0, int32_t y0, int32_t op) {
//     return gh_wrap(golhip_group_stamp_bits(hs, n, words, pw, ph, x0, y0, op));
// }
// static gh_status gh_stamp_file(golhip_t *hs, int32_t n, const char *path, int32_t x0, int32_t y0, int32_t op,
//                                golhip_pattern_info_t *info) {
//     return gh_wrap(golhip_stamp_file(hs, n, path, x0, y0, op, info));
// }
// // Saving patterns (golhip_group_extract_bits, golhip_alive_box, golhip_save_rle):
// // any rectangle read back, the box around the alive cells, an RLE file of either.
// static gh_status gh_group_extract_bits(golhip_t *hs, int32_t n, int32_t x0, int32_t y0, int32_t pw, int32_t ph,
//                                        uint32_t *words, uint64_t cap) {
//     return gh_wrap(golhip_group_extract_bits(hs, n, x0, y0, pw, ph, words, cap));
// }
// static gh_status gh_alive_box(golhip_t *hs, int32_t n, int32_t *x0, int32_t *y0, int32_t *pw, int32_t *ph) {
//     return gh_wrap(golhip_alive_box(hs, n, x0, y0, pw, ph));
// }
// static gh_status gh_save_rle(golhip_t *hs, int32_t n, const char *path, int32_t x0, int32_t y0, int32_t pw,
//                              int32_t ph, int32_t chunk_rows, golhip_pattern_info_t *info) {
//     return gh_wrap(golhip_save_rle(hs, n, path, x0, y0, pw, ph, chunk_rows, info));
// }
// // Life-like rules (golhip_rule_parse, golhip_set_rule): the rule of the turns
// // enqueued from now on, two 9-bit masks; every strip of a group gets the same.
// static gh_status gh_rule_parse(const char *text, uint32_t *birth, uint32_t *survive) {
//     return gh_wrap(golhip_rule_parse(text, birth, survive));
// }
// static gh_status gh_set_rule(golhip_t h, uint32_t birth, uint32_t survive) {
//     return gh_wrap(golhip_set_rule(h, birth, survive));
// }
// // The flip streams of another rule than Conway's (golhip_set_rule_flips): 0 a
// // step and a compaction a turn (the default), 1 the fused turn + list kernel.
// static gh_status gh_set_rule_flips(golhip_t h, int32_t mode) { return gh_wrap(golhip_set_rule_flips(h, mode)); }
// static gh_status gh_rule_flips(golhip_t h, int32_t *mode) { return gh_wrap(golhip_rule_flips(h, mode)); }
// // The padded torus (int golhip_set_pad_step(golhip_t h, int32_t mode)): a width
// // that is no multiple of 32 on the fast kernels; -1 the measured rule (the
// // default, which the engine keeps), 0 never, 1 always.
// static gh_status gh_set_pad_step(golhip_t h, int32_t mode) { return gh_wrap(golhip_set_pad_step(h, mode)); }
// // Padded strips (int golhip_group_set_pad_step(golhip_t *hs, int32_t n, int32_t mode)):
// // the same for the strips of a group; the engine keeps the measured rule.
// static gh_status gh_group_set_pad_step(golhip_t *hs, int32_t n, int32_t mode) {
//     return gh_wrap(golhip_group_set_pad_step(hs, n, mode));
// }
import "C"

import (
	"os"
	"strconv"
	"unsafe"

	"uk.ac.bris.cs/gameoflife/util"
)

// engine is the board of one Run: one libgolhip handle (a whole torus on
// GPU 0) or, with GOL_NGPU=n / GOL_STRIPS=k in the environment (SURVEY 5's
// config row; the README's halo-exchange extension), k row strips on devices
// 0..n-1 (k = n by default) stepped together by golhip_group_step_ex, their
// halo rows moved between the strips' devices by peer copies.  Side channels
// of the strips are gathered in strip order, which is the board's row-major
// order: alive lists and flip lists concatenate, counts add up.
type engine struct {
	hs     []C.golhip_t // one handle per strip, top to bottom
	row0   []int        // first board row of each strip
	width  int
	height int

	flipsP unsafe.Pointer // golhip_host_alloc buffer of cell indices y*width + x
	flips  []uint32       // a Go view of it
	counts []uint64       // per-turn list lengths of the last flipStream

	framesP unsafe.Pointer // golhip_host_alloc buffer of view frames (ARGB8888)
	frames  []uint32       // a Go view of it

	// Rule is the run's Life-like rule as (birth, survive) masks (golhip.h);
	// Conway's B3/S23 unless the package variable Rule names another.
	Rule [2]uint32

	ckpt     *C.golhip_ckpt // the checkpoint in flight (at most one)
	ckptTurn int            // turn of the last checkpoint begun (-1: none)
}

// check turns a libgolhip status into the reference's fail-fast behaviour
// (util.Check panics, the io goroutine panics on a bad PGM); the message came
// back with the status from the same C call (gh_wrap).
func check(s C.gh_status) {
	if s.rc != C.GOLHIP_OK {
		panic("golhip: " + C.GoString(&s.msg[0]))
	}
}

func envInt(name string, dflt int) int {
	if v, err := strconv.Atoi(os.Getenv(name)); err == nil {
		return v
	}
	return dflt
}

// newEngine replaces the world allocation and fill of distributor.go:66-80:
// cells is the raster the io goroutine sent, row-major, alive <=> 255.
func newEngine(p Params, cells []byte) *engine {
	e := createEngine(p)
	for i, h := range e.hs {
		check(C.gh_load_bytes(h, (*C.uint8_t)(unsafe.Pointer(&cells[e.row0[i]*e.width]))))
	}
	return e
}

// resumeEngine is newEngine from a checkpoint file (golhip_checkpoint_load)
// instead of the io goroutine's raster: the board and the turn it is at.  It
// panics where the io goroutine panics on a bad image: another size than
// Params, a turn past Params.Turns, a damaged file.
func resumeEngine(p Params, path string) (*engine, int) {
	cpath := C.CString(path)
	defer C.free(unsafe.Pointer(cpath))
	var info C.golhip_ckpt_info_t
	check(C.gh_checkpoint_info(cpath, &info))
	if int(info.width) != p.ImageWidth {
		panic("Incorrect width")
	}
	if int(info.height) != p.ImageHeight {
		panic("Incorrect height")
	}
	if int(info.turn) > p.Turns {
		panic("checkpoint " + path + " is at turn " + strconv.Itoa(int(info.turn)) + ", past the run's turns")
	}
	e := createEngine(p)
	check(C.gh_checkpoint_load((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), cpath))
	return e, int(info.turn)
}

// streamImages reports GOL_STREAM_IMAGES=1: images/ and out/ files through
// golhip_image_* instead of the io goroutine's whole rasters.
func streamImages() bool { return envInt("GOL_STREAM_IMAGES", 0) != 0 }

// loadImageEngine is newEngine without the io goroutine's raster: the file is
// checked against Params, read, copied and packed chunk by chunk
// (golhip_image_load, whose checks come in the io goroutine's order).  It
// panics with the io goroutine's messages.
func loadImageEngine(p Params, path string) *engine {
	cpath := C.CString(path)
	defer C.free(unsafe.Pointer(cpath))
	e := createEngine(p)
	if s := C.gh_image_load((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), cpath); s.rc != C.GOLHIP_OK {
		e.close()
		panic(C.GoString(&s.msg[0]))
	}
	return e
}

// Stamp ops (GOLHIP_STAMP_*): what a pattern does to the cells of its rectangle.
const (
	StampCopy  = 0 // the rectangle becomes the pattern, dead cells included
	StampOr    = 1 // cells alive in the pattern come alive
	StampXor   = 2 // cells alive in the pattern flip
	StampClear = 3 // cells alive in the pattern die
)

// Clear leaves every cell of the board dead at turn 0 (golhip_clear on every strip).
func (e *engine) Clear() {
	for _, h := range e.hs {
		check(C.gh_clear(h))
	}
}

// StampBits merges a pw x ph pattern of bit words (ph rows of ceil(pw/32)
// words, cell (r, c) = bit c%32 of word c/32 of row r) into the board with its
// top-left corner at the torus cell (x0, y0); the turn does not change
// (golhip_group_stamp_bits).  words is only read during the call.
func (e *engine) StampBits(words []uint32, pw, ph, x0, y0, op int) {
	if len(words) < ph*((pw+31)/32) || len(words) == 0 {
		panic("StampBits: words shorter than the pattern")
	}
	check(C.gh_group_stamp_bits((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)),
		(*C.uint32_t)(unsafe.Pointer(&words[0])), C.int32_t(pw), C.int32_t(ph), C.int32_t(x0), C.int32_t(y0), C.int32_t(op)))
}

// StampFile stamps a pattern file (RLE, or a PGM with alive = 255; told apart
// by the first bytes) and returns its width, height and alive cells
// (golhip_stamp_file).  A file that does not parse or fit panics with the
// parser's message.
func (e *engine) StampFile(path string, x0, y0, op int) (width, height int, alive uint64) {
	cpath := C.CString(path)
	defer C.free(unsafe.Pointer(cpath))
	var info C.golhip_pattern_info_t
	check(C.gh_stamp_file((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), cpath, C.int32_t(x0), C.int32_t(y0),
		C.int32_t(op), &info))
	return int(info.width), int(info.height), uint64(info.alive)
}

// ExtractBits reads the pw x ph cells whose top-left corner is the torus cell
// (x0, y0), wrapping in x and y, as StampBits takes them: ph rows of
// ceil(pw/32) words, padding bits zero (golhip_group_extract_bits).  The board
// is not written; turn, count and flip list stay.
func (e *engine) ExtractBits(x0, y0, pw, ph int) []uint32 {
	if pw < 1 || ph < 1 {
		panic("ExtractBits: sizes start at 1")
	}
	words := make([]uint32, ph*((pw+31)/32))
	check(C.gh_group_extract_bits((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), C.int32_t(x0), C.int32_t(y0),
		C.int32_t(pw), C.int32_t(ph), (*C.uint32_t)(unsafe.Pointer(&words[0])), C.uint64_t(len(words))))
	return words
}

// AliveBox is the smallest box of at most one lap around every alive cell of
// the torus, seams included; pw = ph = 0 on an empty board (golhip_alive_box).
func (e *engine) AliveBox() (x0, y0, pw, ph int) {
	var cx, cy, cw, ch C.int32_t
	check(C.gh_alive_box((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), &cx, &cy, &cw, &ch))
	return int(cx), int(cy), int(cw), int(ch)
}

// SaveRle writes the rectangle (pw = ph = 0: the alive box) as an RLE file
// whose header names the run's rule, a chunk of rows at a time, and returns its
// width, height and alive cells (golhip_save_rle).  ok is false, and no file is
// written, where the alive box was asked for and the board is empty.
func (e *engine) SaveRle(path string, x0, y0, pw, ph int) (width, height int, alive uint64, ok bool) {
	if pw == 0 && ph == 0 {
		if _, _, w, _ := e.AliveBox(); w == 0 {
			return 0, 0, 0, false
		}
	}
	cpath := C.CString(path)
	defer C.free(unsafe.Pointer(cpath))
	var info C.golhip_pattern_info_t
	check(C.gh_save_rle((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), cpath, C.int32_t(x0), C.int32_t(y0),
		C.int32_t(pw), C.int32_t(ph), 0, &info))
	return int(info.width), int(info.height), uint64(info.alive), true
}

// imageBegin starts the image of the board at its current turn
// (golhip_image_begin: the caller holds the run's mutex for this call only);
// imageWait joins it: the file is complete, or the run panics with the error.
func (e *engine) imageBegin(path string) *C.golhip_image {
	cpath := C.CString(path)
	defer C.free(unsafe.Pointer(cpath))
	var im *C.golhip_image
	check(C.gh_image_begin((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), cpath, &im))
	return im
}

func imageWait(im *C.golhip_image) { check(C.gh_image_wait(im)) }

// checkpointBegin starts a checkpoint of the board at its current turn
// (golhip_checkpoint_begin: one kernel a strip behind the turns enqueued; the
// file drains behind the following turns), after waiting for the previous one.
func (e *engine) checkpointBegin(path string, turn int) {
	e.checkpointWait()
	cpath := C.CString(path)
	defer C.free(unsafe.Pointer(cpath))
	check(C.gh_checkpoint_begin((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), cpath, &e.ckpt))
	e.ckptTurn = turn
}

// checkpointWait joins the checkpoint in flight: its file is complete, or the
// run panics with the file error.
func (e *engine) checkpointWait() {
	if e.ckpt != nil {
		ck := e.ckpt
		e.ckpt = nil
		check(C.gh_checkpoint_wait(ck))
	}
}

// Rule is the Life-like rule of the runs of this process, in any spelling
// golhip_rule_parse takes ("B36/S23", "23/36"); empty: Conway's B3/S23, or the
// environment's GOL_RULE.  The reference's Params has no field to carry it.  A
// run from a checkpoint names it again: the file keeps none.
var Rule string

// SetRule sets the rule on every handle of the engine (golhip_set_rule); a
// spelling that does not parse panics with the parser's message.
func (e *engine) SetRule(text string) {
	ctext := C.CString(text)
	defer C.free(unsafe.Pointer(ctext))
	var b, s C.uint32_t
	check(C.gh_rule_parse(ctext, &b, &s))
	fused := C.int32_t(0)
	if envInt("GOL_RULE_FLIPS", 0) != 0 {
		fused = 1 // the CellFlipped batches from the fused turn + list kernel; the same events
	}
	for _, h := range e.hs {
		check(C.gh_set_rule(h, b, s))
		check(C.gh_set_rule_flips(h, fused))
	}
	e.Rule = [2]uint32{uint32(b), uint32(s)}
}

// createEngine makes the handles of newEngine / resumeEngine (no board yet).
func createEngine(p Params) *engine {
	e := &engine{width: p.ImageWidth, height: p.ImageHeight, ckptTurn: -1, Rule: [2]uint32{0x008, 0x00C}}
	defer func() {
		rule := Rule
		if rule == "" {
			rule = os.Getenv("GOL_RULE")
		}
		if rule != "" && len(e.hs) > 0 {
			e.SetRule(rule)
		}
	}()
	ngpu := envInt("GOL_NGPU", 1)
	n := envInt("GOL_STRIPS", 0)
	if n <= 0 {
		n = ngpu
	}
	if n > p.ImageHeight {
		n = p.ImageHeight
	}
	if n <= 1 {
		var h C.golhip_t
		check(C.gh_create(C.int32_t(p.ImageWidth), C.int32_t(p.ImageHeight), &h))
		e.hs, e.row0 = []C.golhip_t{h}, []int{0}
	} else {
		var ndev C.int32_t
		check(C.gh_device_count(&ndev))
		devs := ngpu
		if devs > int(ndev) {
			devs = int(ndev)
		}
		if devs < 1 {
			devs = 1
		}
		for i := 0; i < n; i++ {
			r0, r1 := p.ImageHeight*i/n, p.ImageHeight*(i+1)/n
			var h C.golhip_t
			st := C.gh_create_strip(C.int32_t(p.ImageWidth), C.int32_t(p.ImageHeight), C.int32_t(r0),
				C.int32_t(r1-r0), C.int32_t(i%devs), &h)
			if st.rc != C.GOLHIP_OK {
				e.close()
				check(st)
			}
			e.hs = append(e.hs, h)
			e.row0 = append(e.row0, r0)
		}
	}
	return e
}

func (e *engine) close() {
	if e.ckpt != nil {
		C.golhip_checkpoint_wait(e.ckpt, nil)
		e.ckpt = nil
	}
	if e.flipsP != nil {
		C.golhip_host_free(e.flipsP)
		e.flipsP = nil
		e.flips = nil
	}
	if e.framesP != nil {
		C.golhip_host_free(e.framesP)
		e.framesP = nil
		e.frames = nil
	}
	for i, h := range e.hs {
		if h != nil {
			C.golhip_destroy(h)
			e.hs[i] = nil
		}
	}
}

// group is the strips' handle array for golhip_group_step_ex (Go memory
// holding C pointers only, valid for the call).
func (e *engine) group(turns int, wantFlips int) {
	check(C.gh_group_step_ex((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), C.int64_t(turns),
		C.int32_t(wantFlips)))
}

// step runs n turns in fused launches (no per-turn side channels).
func (e *engine) step(n int) {
	if len(e.hs) == 1 {
		check(C.gh_step_sync(e.hs[0], C.int64_t(n)))
		return
	}
	e.group(n, 0)
}

func (e *engine) growFlips(n int) {
	if n <= len(e.flips) {
		return
	}
	if e.flipsP != nil {
		C.golhip_host_free(e.flipsP)
		e.flipsP = nil
		e.flips = nil
	}
	var p unsafe.Pointer
	check(C.gh_host_alloc(C.uint64_t(n*4), &p))
	e.flipsP = p
	e.flips = (*[1 << 32]uint32)(p)[:n:n]
}

// flipStream runs up to n turns, each with its CellFlipped list
// (initializeAliveCells, distributor.go:212-220), and returns how many ran,
// each turn's list length and the lists concatenated in turn order: cell
// indices y*width + x, row-major within a turn.  The batch stops early rather
// than drop an entry; the views are valid until the next call.
func (e *engine) flipStream(n int) (int, []uint64, []uint32) {
	if e.flipsP == nil {
		first := e.width * e.height // one turn flips at most every cell
		if first > 16<<20 {
			first = 16 << 20
		}
		e.growFlips(first)
	}
	if len(e.counts) < n {
		e.counts = make([]uint64, n)
	}
	var done C.int64_t
	var total C.uint64_t
	call := func() C.gh_status {
		if len(e.hs) > 1 { // row strips: the same contract on the whole board (golhip_group_flip_stream)
			return C.gh_group_flip_stream((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), C.int64_t(n),
				e.flipsP, C.uint64_t(len(e.flips)), (*C.uint64_t)(unsafe.Pointer(&e.counts[0])), &done, &total)
		}
		return C.gh_flip_stream(e.hs[0], C.int64_t(n), e.flipsP, C.uint64_t(len(e.flips)),
			(*C.uint64_t)(unsafe.Pointer(&e.counts[0])), &done, &total)
	}
	st := call()
	if st.rc == C.GOLHIP_ERANGE { // the next turn alone needs `total` entries; nothing advanced
		e.growFlips(int(total))
		st = call()
	}
	check(st)
	return int(done), e.counts[:int(done)], e.flips[:int(total)]
}

// aliveCells is calculateAliveCells (distributor.go:420-432): Cell{X: col, Y: row}, row-major.
func (e *engine) aliveCells() []util.Cell {
	cells := []util.Cell{}
	for _, h := range e.hs {
		var n C.uint64_t
		if st := C.gh_alive_cells(h, nil, 0, &n); st.rc != C.GOLHIP_OK && st.rc != C.GOLHIP_ERANGE {
			check(st)
		}
		if n == 0 {
			continue
		}
		xy := make([]int32, 2*int(n))
		check(C.gh_alive_cells(h, (*C.int32_t)(unsafe.Pointer(&xy[0])), n, &n))
		for i := 0; i < int(n); i++ {
			cells = append(cells, util.Cell{X: int(xy[2*i]), Y: int(xy[2*i+1])})
		}
	}
	return cells
}

// aliveCount is the ticker's len(calculateAliveCells(world)) (:292) with the
// turn it belongs to, read together (the reference reads *turn unlocked, :294);
// strips add their counts (all at the same turn: the caller holds mu).
func (e *engine) aliveCount() (turn int, count int) {
	for _, h := range e.hs {
		var n C.uint64_t
		var t C.int64_t
		check(C.gh_alive_count(h, &n, &t))
		turn, count = int(t), count+int(n)
	}
	return turn, count
}

// snapshot is the board as the 0/255 raster the io goroutine writes (:186-191).
func (e *engine) snapshot() []byte {
	out := make([]byte, e.width*e.height)
	for i, h := range e.hs {
		check(C.gh_snapshot_bytes(h, (*C.uint8_t)(unsafe.Pointer(&out[e.row0[i]*e.width]))))
	}
	return out
}

// View is the window onto the board (golhip_view_t): Scale x Scale cells a
// pixel from cell (X0, Y0) on, OutW x OutH ARGB8888 pixels (the texture format
// of sdl/window.go:32).  At Scale 1 a frame is the pixel buffer of the
// reference's Window after its flips.
type View struct {
	X0, Y0, Scale, OutW, OutH int
}

func (v View) c() C.golhip_view_t {
	return C.golhip_view_t{x0: C.int32_t(v.X0), y0: C.int32_t(v.Y0), scale: C.int32_t(v.Scale),
		out_w: C.int32_t(v.OutW), out_h: C.int32_t(v.OutH), format: C.GOLHIP_VIEW_ARGB8888}
}

// growFrames makes the page-locked frame buffer hold n frames of v (C memory
// the view kernel writes itself, like the flip buffer).
func (e *engine) growFrames(v View, n int) {
	need := n * v.OutW * v.OutH
	if need <= len(e.frames) {
		return
	}
	if e.framesP != nil {
		C.golhip_host_free(e.framesP)
		e.framesP = nil
		e.frames = nil
	}
	var p unsafe.Pointer
	check(C.gh_host_alloc(C.uint64_t(need*4), &p))
	e.framesP = p
	e.frames = (*[1 << 32]uint32)(p)[:need:need]
}

// ViewFrame renders the current board through v and returns the pixels and
// the turn they show; the slice is valid until the next view call.  One strip
// only (a whole-torus handle).
func (e *engine) ViewFrame(v View) ([]uint32, int) {
	e.growFrames(v, 1)
	cv := v.c()
	var turn C.int64_t
	check(C.gh_view_frame(e.hs[0], &cv, e.framesP, C.uint64_t(len(e.frames)*4), &turn))
	return e.frames[:v.OutW*v.OutH], int(turn)
}

// ViewStream runs n turns with a frame behind every `every`-th and returns
// the n / every frames, consecutive, each OutW*OutH pixels (frame i shows turn
// (i+1)*every of the batch); the slice is valid until the next view call.
func (e *engine) ViewStream(n int, every int, v View) []uint32 {
	e.growFrames(v, n/every)
	cv := v.c()
	var frames C.uint64_t
	var done C.int64_t
	check(C.gh_view_stream(e.hs[0], C.int64_t(n), C.int64_t(every), &cv, e.framesP,
		C.uint64_t(len(e.frames)/(v.OutW*v.OutH)), &frames, &done))
	return e.frames[:int(frames)*v.OutW*v.OutH]
}

// GroupViewFrame is ViewFrame on every strip of the engine
// (golhip_group_view_frame): the viewport may cross strip boundaries and both
// seams.  On one whole-torus handle it is ViewFrame.
func (e *engine) GroupViewFrame(v View) ([]uint32, int) {
	e.growFrames(v, 1)
	cv := v.c()
	var turn C.int64_t
	check(C.gh_group_view_frame((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), &cv, e.framesP, C.uint64_t(len(e.frames)*4), &turn))
	return e.frames[:v.OutW*v.OutH], int(turn)
}

// GroupViewStream is ViewStream on every strip of the engine
// (golhip_group_view_stream).
func (e *engine) GroupViewStream(n int, every int, v View) []uint32 {
	e.growFrames(v, n/every)
	cv := v.c()
	var frames C.uint64_t
	var done C.int64_t
	check(C.gh_group_view_stream((*C.golhip_t)(unsafe.Pointer(&e.hs[0])), C.int32_t(len(e.hs)), C.int64_t(n), C.int64_t(every), &cv, e.framesP,
		C.uint64_t(len(e.frames)/(v.OutW*v.OutH)), &frames, &done))
	return e.frames[:int(frames)*v.OutW*v.OutH]
}
