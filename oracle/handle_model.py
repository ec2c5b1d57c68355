"""A numpy model of one golhip handle (or of a group of row strips) and a
seeded driver that runs call sequences against it -- TEST INFRASTRUCTURE ONLY.

What the per-feature suites do not reach is the handle as a state machine: one
entry point leaves state (the current buffer, the word layout, the kept count,
the flip list, scratch that several calls share, a shadow in flight) and a
different one consumes it.  Here a model answers every call with the value or
the GOLHIP_E* code that include/golhip.h documents, a driver draws calls from
a weighted table with a seeded numpy generator, applies each to the model and
to a target, and compares.

* ``HandleModel`` -- the board as 0/255 bytes, the turn, the rule, the flip list
  (the two boards it is the difference of), the jobs begun and not yet waited
  for.  Built from oracle.oracle (run_np, step_np, flips_np, alive_cells_np,
  pack_bits, fill_random_np) and golhip's numpy restatements (stamp_np,
  view_frame_np, board_hash_np, checkpoint_*_np, life_like_np, extract_np,
  alive_box_np, rle_parse_np, rle_format_np).  Where the header is silent
  the model says nothing: the flip list is then UNKNOWN and the driver does not
  ask for it.  Nothing here is copied from the library's host code.
* ``BoardTarget`` / ``GroupTarget`` -- the same calls on a golhip.Board and on
  a list of strips (the group entry points; rows concatenated, counts and
  digests summed, every strip's turn reported).
* ``run_sequence`` -- the driver.  No clock, no retry; a mismatch raises
  ``SequenceMismatch`` with the calls so far as a block of ``hm.replay`` lines
  that runs as pasted (tests/test_sequences_cpu.py executes one).

The model doubles as the fake target of tests/test_sequences_cpu.py
(``fake=True``: it writes the files of its jobs), where ``defect`` names one
one-line defect of the fake that the committed seeds must catch.
"""
from __future__ import annotations

import os
import re

import numpy as np

import golhip as G  # the numpy restatements; the library is loaded by the targets alone
from oracle.oracle import (alive_cells_np, fill_random_np, flips_np, pack_bits, pgm_bytes, read_pgm, run_np, step_np,
                           unpack_bits)

OK, EINVAL, ERANGE = 0, -1, -4
UNKNOWN = "unknown"  # the header does not say whether the handle keeps a flip list
CONWAY = (0x008, 0x00C)  # (birth, survive): bit n of each for n alive neighbours
# the rules with a static instance of the rule kernel K11 besides Conway's, and three that take its dynamic policy
STATIC_RULES = {"B36/S23": (0x048, 0x00C), "B3678/S34678": (0x1C8, 0x1D8), "B2/S": (0x004, 0x000),
                "B3/S012345678": (0x008, 0x1FF), "B1357/S1357": (0x0AA, 0x0AA), "B36/S125": (0x048, 0x026)}
DYNAMIC_RULES = {"B3578/S1246": (0x1A8, 0x056), "B0/S8": (0x001, 0x100), "B012345678/S": (0x1FF, 0x000)}


class Refused(Exception):
    """A call answered with a GOLHIP_E* code (need: the size an ERANGE reports)."""

    def __init__(self, code: int, need: int | None = None):
        super().__init__(f"refused with {code}" + (f" (needs {need})" if need is not None else ""))
        self.code, self.need = code, need


class SequenceMismatch(AssertionError):
    """The target and the model disagree.  str(): what differed, then the calls
    so far as a block of Python lines that replays them on a fresh target (the
    last line is the call that differed: its value is `got`)."""
    lines: list = []
    got = None


# --------------------------------------------------------------------------- reproducible arguments
class Cells:
    """An array argument that a replay line can rebuild: kind "board" (H x W
    bytes, 255 alive; mode 0 dense, 1 sparse, 2 dense with dead cells written as
    other non-255 bytes), "words" (bit words of such a board; dirty: the bits of
    columns >= W set), "pattern" (ph x pw bools)."""

    def __init__(self, kind: str, *a: int):
        self.kind, self.a = kind, tuple(int(x) for x in a)

    def __repr__(self):
        return f"hm.Cells({self.kind!r}, {', '.join(map(str, self.a))})"

    @staticmethod
    def _board(W, H, seed, mode):
        b = fill_random_np(W, H, seed)
        if mode == 1:
            b = b & fill_random_np(W, H, seed + 1) & fill_random_np(W, H, seed + 2)
        if mode == 2:
            junk = (fill_random_np(W, H, seed + 3) == 255) & (b == 0)
            b = np.where(junk, np.uint8(1 + seed % 254), b).astype(np.uint8)
        return b

    def make(self) -> np.ndarray:
        if self.kind == "board":
            return self._board(*self.a)
        if self.kind == "words":
            W, H, seed, mode, dirty = self.a
            w = pack_bits(self._board(W, H, seed, mode))
            if dirty and W % 32:
                w[:, -1] |= np.uint32((0xFFFFFFFF << (W % 32)) & 0xFFFFFFFF)
            return w
        if self.kind == "pattern":
            pw, ph, seed = self.a
            return np.random.default_rng(seed).random((ph, pw)) < 0.5
        raise ValueError(self.kind)


def write_ckpt(path: str, cells: Cells, turn: int) -> None:
    """A checkpoint file from numpy alone (golhip.checkpoint_write_np)."""
    b = cells.make()
    G.checkpoint_write_np(path, pack_bits(np.where(b == 255, 255, 0).astype(np.uint8)), b.shape[1], b.shape[0], turn)


def write_pgm(path: str, cells: Cells) -> None:
    with open(path, "wb") as f:
        f.write(pgm_bytes(cells.make()))


def rule_text(rule) -> str:
    """The canonical spelling of (birth, survive): "B36/S23", digits ascending."""
    b, s = rule
    return "B" + "".join(str(n) for n in range(9) if b >> n & 1) + "/S" + "".join(str(n) for n in range(9) if s >> n & 1)


def rule_of_text(text: str):
    """(birth, survive) of "B<digits>/S<digits>" (either case) or the legacy "<survive>/<birth>"."""
    t = text.strip().upper()
    if t.startswith("B"):
        b, s = t[1:].split("/S")
    else:
        s, b = t.split("/")
    return (sum(1 << int(c) for c in b), sum(1 << int(c) for c in s))


_RLE_HEAD = re.compile(r"(?m)^(\s*x\s*=\s*\d+\s*,\s*y\s*=\s*\d+)\s*,\s*rule\s*=\s*(\S+)\s*$")


def rle_split(text: str):
    """(the rule an RLE text's header names or None, the text without it)."""
    m = _RLE_HEAD.search(text)
    if not m:
        return None, text
    return rule_of_text(m.group(2)), text[:m.start()] + m.group(1) + text[m.end():]


def write_rle(path: str, cells: Cells, rule) -> None:
    """An RLE file of the pattern whose header names `rule` (golhip_pattern_write; no device)."""
    G.pattern_write(path, cells.make(), tuple(rule))


def write_text(path: str, text: str) -> None:
    with open(path, "w") as f:
        f.write(text)


def replay(target, method, *args, **kwargs):
    """One call as the driver makes it, and as its printed lines make it again:
    Cells arguments are built, and the answer is ("ok", value) or ("refused",
    code, need) -- a refused call does not end a pasted block."""
    real = tuple(a.make() if isinstance(a, Cells) else a for a in args)
    try:
        return ("ok", getattr(target, method)(*real, **kwargs))
    except Refused as e:
        return ("refused", e.code, e.need)


def _alive(board: np.ndarray) -> int:
    return int(np.count_nonzero(board == 255))


def _entries(xy: np.ndarray, fmt: int, W: int) -> np.ndarray:
    if fmt == G.FLIPS_XY:
        return xy.astype(np.int32).reshape(-1, 2)
    return (xy[:, 1].astype(np.uint64) * np.uint64(W) + xy[:, 0].astype(np.uint64)).astype(np.uint32)


# --------------------------------------------------------------------------- the model
class HandleModel:
    """One whole-torus handle (cuts None) or the group of strips
    [cuts[i], cuts[i + 1]) of one board, as include/golhip.h documents them."""

    def __init__(self, W: int, H: int, cuts=None, run=run_np, fake: bool = False, defect: str | None = None):
        self.W, self.H = W, H
        self.cuts = list(cuts) if cuts is not None else None
        self.run = run
        self.fake, self.defect = fake, defect
        self.board: np.ndarray | None = None
        self.t = 0
        self.flip = None       # None: no list (EINVAL) | UNKNOWN | (board before, board after)
        self.fresh = False     # the board was replaced and no flip batch has run on it since
        self.jobs: dict[int, tuple] = {}
        self.njobs = 0
        self._count = None     # the fake's kept alive count
        self._behind = False   # the fake's defect "strip_behind"
        self.rule = CONWAY     # (birth, survive) of the turns stepped from now on
        self._lag = None       # the fake's defect "rule_lags_a_call": the rule the next stepping call still runs

    @property
    def nstrips(self) -> int:
        return 1 if self.cuts is None else len(self.cuts) - 1

    # ---- the rule
    def set_rule(self, rule):
        b, s = rule
        if not (0 <= b <= 0x1FF and 0 <= s <= 0x1FF):
            raise Refused(EINVAL)  # the rule is then unchanged
        if self.defect == "rule_lags_a_call" and (b, s) != self.rule:
            self._lag = self.rule
        if self.defect == "set_rule_drops_flips":
            self.flip = None
        self.rule = (int(b), int(s))  # board, turn, kept count, flip list and jobs stay

    def _run(self, board, n, rule=None):
        rule = rule or self._lag or self.rule
        return self.run(board, n) if rule == CONWAY else G.life_like_np(board, rule[0], rule[1], n)

    def _step1(self, board, rule=None):
        rule = rule or self._lag or self.rule
        return step_np(board) if rule == CONWAY else G.life_like_np(board, rule[0], rule[1], 1)

    # ---- board replaced
    def _replace(self, board, turn=0):
        self.board = np.where(board == 255, 255, 0).astype(np.uint8)
        self.t, self.flip, self.fresh, self._count, self._behind = turn, None, True, None, False

    def load_bytes(self, cells):
        self._replace(cells)

    def load_bits(self, words):
        self._replace(unpack_bits(np.ascontiguousarray(words, dtype=np.uint32), self.W))

    def fill_random(self, seed):
        self._replace(fill_random_np(self.W, self.H, seed))

    def clear(self):
        t = self.t
        self._replace(np.zeros((self.H, self.W), dtype=np.uint8))
        if self.defect == "clear_keeps_turn":
            self.t = t

    def checkpoint_load(self, path):
        info, words = G.checkpoint_read_np(path)
        if (info["width"], info["height"]) != (self.W, self.H):
            raise Refused(EINVAL)
        self._replace(unpack_bits(words, self.W), info["turn"])
        return {"turn": info["turn"], "alive": info["alive"]}

    def image_load(self, path):
        try:
            b = read_pgm(path, self.W, self.H)
        except ValueError:
            raise Refused(EINVAL) from None
        self._replace(b)
        return {"alive": _alive(self.board)}

    # ---- board edited
    def stamp(self, cells, x0, y0, op, strip=None):
        c = np.asarray(cells, dtype=bool)
        ph, pw = c.shape if c.ndim == 2 else (0, 0)
        if not (0 <= x0 < self.W and 0 <= y0 < self.H and 1 <= pw <= self.W and 1 <= ph <= self.H and 0 <= op <= 3):
            raise Refused(EINVAL)  # the board is then unchanged
        if self.defect == "stamp_drops_columns" and x0 + pw > self.W:
            c = c[:, :self.W - x0]
        if self.defect == "stamp_drops_rows" and y0 + ph > self.H:
            c = c[:self.H - y0]
        new = G.stamp_np(self.board, c, x0, y0, op)
        if strip is not None:  # a stamp on one strip alone takes the rows that strip owns
            a, b = self.cuts[strip], self.cuts[strip + 1]
            new[:a], new[b:] = self.board[:a], self.board[b:]
        self.board = new
        if self.defect != "count_kept_over_stamp":
            self._count = None
        if self.cuts is not None:
            self.flip = UNKNOWN  # (which strips of a group drop their lists: the header is silent)
        elif self.defect != "flips_kept_over_stamp":
            self.flip = None

    def stamp_file(self, path, x0, y0, op):
        """golhip_stamp_file of an RLE file: it must name the handle's rule or
        none (on a Conway handle that is golhip_pattern_info's check); then
        the stamp of its cells."""
        with open(path) as f:
            named, text = rle_split(f.read())
        if named is not None and named != self.rule and self.defect != "stamp_file_any_rule":
            raise Refused(EINVAL)  # the board is then unchanged
        cells = G.rle_parse_np(text)
        self.stamp(cells, x0, y0, op)
        return {"width": cells.shape[1], "height": cells.shape[0], "alive": int(cells.sum()), "format": "rle"}

    # ---- turns
    def _advance(self, n, want_flips=False):
        if n == 0:
            self.flip = UNKNOWN  # no turn was stepped: the header is silent
            return
        if want_flips:
            prev = self._run(self.board, n - 1)
            self.board = self._step1(prev)
            self.flip = (prev, self.board)
        else:
            self.board = self._run(self.board, n)
            self.flip = None
        self.t += n
        self._count = None

    def step(self, n, want_flips=False):
        self._advance(n, want_flips)
        if n > 0:
            self._lag = None

    def _lists(self, n):
        b = self.board
        rule = CONWAY if self.defect == "stream_steps_conway" else None
        for _ in range(n):
            nb = self._step1(b, rule)
            yield nb, flips_np(b, nb)
            b = nb

    def step_flips(self, n, cap):
        """(code, the first cap pairs, counts, total): the board always advances n."""
        lists, last = [], self.board
        for last, l in self._lists(n):
            lists.append(l)
        self.board, self.t, self.flip = last, self.t + n, None if n > 0 else UNKNOWN
        self.fresh, self._count = self.fresh and n == 0, None
        if n > 0:
            self._lag = None
        xy = np.concatenate(lists).reshape(-1, 2) if lists else np.zeros((0, 2), np.int32)
        return (ERANGE if len(xy) > cap else OK, xy[:cap].astype(np.int32), [len(l) for l in lists], len(xy))

    def flip_stream(self, n, cap, fmt, pinned=False, done=None):
        """(entries, counts, turns done, entries written); ERANGE with nothing
        advanced when the first list does not fit.  `done`: what the target
        reported -- a batch may stop short of a turn that fits, but not the first
        batch on a replaced board."""
        if n == 0:
            self.flip = UNKNOWN
            return (_entries(np.zeros((0, 2), np.int32), fmt, self.W), [], 0, 0)
        boards, lists, used = [], [], 0
        for nb, l in self._lists(n):
            if used + len(l) > cap:
                if not lists:
                    self.flip = UNKNOWN
                    if self.defect == "stream_advances_on_erange":
                        self.board, self.t, self._count = nb, self.t + 1, None
                    raise Refused(ERANGE, len(l))
                break
            used += len(l)
            boards.append(nb)
            lists.append(l)
        fit = len(lists)
        if done is None:
            done = fit
        if not 1 <= done <= fit:
            raise SequenceMismatch(f"flip stream ran {done} turns, the contract allows 1..{fit}")
        if self.fresh and done != fit:
            raise SequenceMismatch(f"first flip batch on a replaced board ran {done} turns, {fit} of {n} fit in {cap}")
        self.fresh = False
        before = boards[done - 2] if done > 1 else self.board
        self.board, self.t, self.flip, self._count = boards[done - 1], self.t + done, None, None
        if self.defect == "rule_stream_keeps_flips" and self.cuts is not None and self.rule != CONWAY and done == n:
            self.flip = (before, self.board)
        self._lag = None
        xy = np.concatenate(lists[:done]).reshape(-1, 2)
        ent = _entries(xy, fmt, self.W)
        if self.defect == "stream_drops_last" and done < n and len(ent):
            ent = ent[:-1]
        if self.defect == "strip_behind" and done < n:
            self._behind = True
        return (ent, [len(l) for l in lists[:done]], done, len(xy))

    def _frame(self, board, v):
        x0, y0, s, ow, oh, fmt = v
        return G.view_frame_np(pack_bits(board), self.W, self.H, x0, y0, s, ow, oh, fmt)

    def view_stream(self, n, every, view, cap_frames):
        """(frames, turns done); ERANGE with nothing advanced when the frames exceed cap_frames."""
        nf = n // every
        if nf > cap_frames:
            raise Refused(ERANGE)
        frames = []
        for _ in range(nf):
            self._advance(every)
            frames.append(self._frame(self.board, view))
        if n - nf * every > 0 or n == 0:
            self._advance(n - nf * every)
        if n > 0:
            self._lag = None
        dt = np.uint8 if view[5] == G.VIEW_GRAY8 else np.uint32
        return (np.stack(frames) if frames else np.zeros((0, view[4], view[3]), dt), n)

    # ---- plan changes: results never depend on them
    def set_option(self, key, value):
        ok = {"wpl": (0, 1, 2, 4), "persistent": (-1, 0, 1), "lds_band": (-1, 0, 1), "skew": (0, 1, 2),
              "timing": (0, 1), "flip_overlap": (0, 1, 2, 3)}
        if key not in ok or value not in ok[key]:
            raise Refused(EINVAL)

    def set_tb_depth(self, turns):
        if not 1 <= turns <= G.MAX_TB_DEPTH:
            raise Refused(EINVAL)

    def set_rows_per_wave(self, rows):
        if rows < 0:
            raise Refused(EINVAL)

    def set_pad_step(self, mode):
        if mode not in (-1, 0, 1) or (mode == 1 and self.W % 32 == 0):
            raise Refused(EINVAL)

    def perf_reset(self):
        pass

    def perf(self):
        return None  # no kernels here

    # ---- observers
    def turn(self):
        if self.cuts is None:
            return self.t
        return (self.t,) * (self.nstrips - 1) + (self.t - 1 if self._behind else self.t,)

    def alive_count(self):
        if not self.fake or self._count is None:
            self._count = _alive(self.board)
        return (self._count, self.turn())

    def board_hash(self):
        return G.board_hash_np(pack_bits(self.board))

    def snapshot_bytes(self):
        return self.board.copy()

    def snapshot_bits(self):
        w = pack_bits(self.board)
        if self.defect == "padding_bit_set" and self.W % 32:
            w[-1, -1] |= np.uint32(1 << 31)
        return w

    def snapshot_rows(self, row, nrows, strip=None):
        a = 0 if strip is None else self.cuts[strip]
        return pack_bits(self.board)[a + row:a + row + nrows]

    def alive_cells(self):
        return alive_cells_np(self.board)

    def flips(self):
        if self.flip is None or self.flip == UNKNOWN:  # (UNKNOWN: only a fake that has left the model's path)
            raise Refused(EINVAL)
        return flips_np(*self.flip)

    def view_frame(self, view):
        return (self._frame(self.board, view), self.t)

    def _rect(self, x0, y0, w, h):
        if not (0 <= x0 < self.W and 0 <= y0 < self.H and 1 <= w <= self.W and 1 <= h <= self.H):
            raise Refused(EINVAL)

    def extract(self, x0, y0, w, h):
        self._rect(x0, y0, w, h)
        cells = G.extract_np(self.board, x0, y0, w, h)
        if self.defect == "extract_no_x_wrap" and x0 + w > self.W:
            cells = cells.copy()
            cells[:, self.W - x0:] = False
        if self.defect == "extract_drops_flips":
            self.flip = None
        return cells

    def alive_box(self):
        if self.defect == "box_not_cyclic" and _alive(self.board):
            ys, xs = np.nonzero(self.board == 255)
            return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))
        return tuple(int(v) for v in G.alive_box_np(self.board))

    def save_rle(self, path, box=None, chunk_rows=0):
        """The info dict of the writer; the file itself is the driver's to check
        (the fake writes it: the documented header lines and rle_format_np's body)."""
        if box is None:
            box = tuple(int(v) for v in G.alive_box_np(self.board))
            if box[2] == 0:
                raise Refused(EINVAL)  # an empty board: no file
        self._rect(*box)
        cells = G.extract_np(self.board, *box)
        if self.fake:
            rule = CONWAY if self.defect == "rle_names_conway" else self.rule
            body = G.rle_format_np(cells).split("\n", 1)[1]
            with open(path, "w") as f:
                f.write(f"#CXRLE Pos={box[0]},{box[1]} Gen={self.t}\n"
                        f"x = {box[2]}, y = {box[3]}, rule = {rule_text(rule)}\n{body}")
        return {"width": box[2], "height": box[3], "alive": int(cells.sum()), "format": "rle"}

    def split_rule(self, strip, rule, what, args):
        """One strip of the group on another rule, one group call, the strip set
        back: (the call's code, whether a file of its was written).  Every call
        that takes a group refuses strips that disagree on the rule."""
        if self.defect == "split_rule_steps" and what == "step":
            self._advance(*args)
            return (OK, False)
        return (EINVAL, False)

    # ---- jobs in flight
    def _begin(self, kind, path):
        self.njobs += 1
        self.jobs[self.njobs] = (kind, path, self.board.copy(), self.t)
        return self.njobs

    def checkpoint_begin(self, path):
        return self._begin("ckpt", path)

    def image_begin(self, path):
        return self._begin("image", path)

    def wait(self, job):
        kind, path, board, turn = self.jobs.pop(job)
        if self.fake:  # the fake writes its file here, from the board as it was at begin
            if self.defect == "shadow_sees_later_edits":
                board = self.board
            if kind == "ckpt":
                G.checkpoint_write_np(path, pack_bits(board), self.W, self.H, turn)
            else:
                with open(path, "wb") as f:
                    f.write(pgm_bytes(board))
        return {"width": self.W, "height": self.H, "turn": turn, "alive": _alive(board)}

    def job_expect(self, job):
        """(kind, path, board, turn) the file of a job must hold."""
        return self.jobs[job]

    def close(self):
        self.jobs.clear()


# --------------------------------------------------------------------------- the targets
def _refusing(fn, *a, **k):
    try:
        return fn(*a, **k)
    except G.GolHipError as e:
        raise Refused(e.code) from None


class _Target:
    """What BoardTarget and GroupTarget share: the job table and the flip-stream call."""

    def _init_jobs(self):
        self.jobs, self.njobs = {}, 0

    def _begin(self, obj):
        self.njobs += 1
        self.jobs[self.njobs] = obj
        return self.njobs

    def wait(self, job):
        info = _refusing(self.jobs.pop(job).wait)
        return {k: info[k] for k in ("width", "height", "turn", "alive")}

    def _stream(self, call, n, cap, fmt, pinned):
        import ctypes
        shape, dt = ((max(cap, 1), 2), np.int32) if fmt == G.FLIPS_XY else ((max(cap, 1),), np.uint32)
        out = G.host_array(shape, dt) if pinned else np.empty(shape, dtype=dt)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        done, tot = ctypes.c_int64(), ctypes.c_uint64()
        rc = call(n, fmt, ctypes.c_void_p(out.ctypes.data), cap, ctypes.c_void_p(counts.ctypes.data),
                  ctypes.byref(done), ctypes.byref(tot))
        if rc != OK:
            raise Refused(rc, tot.value)
        return (np.array(out[:tot.value]), [int(c) for c in counts[:done.value]], done.value, tot.value)

    def close(self):
        for j in list(self.jobs):
            try:
                self.wait(j)
            except Exception:  # noqa: BLE001 - closing after a mismatch
                pass


class BoardTarget(_Target):
    """HandleModel's calls on one golhip.Board."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.b = G.Board(W, H)
        self._init_jobs()

    def close(self):
        super().close()
        self.b.close()

    def _handles(self):
        return [self.b]

    def load_bytes(self, cells):
        _refusing(self.b.load_bytes, cells)

    def load_bits(self, words):
        _refusing(self.b.load_bits, words)

    def fill_random(self, seed):
        _refusing(self.b.fill_random, seed)

    def clear(self):
        _refusing(self.b.clear)

    def checkpoint_load(self, path):
        d = _refusing(G.checkpoint_load, self._handles(), path)
        return {"turn": d["turn"], "alive": d["alive"]}

    def image_load(self, path):
        return {"alive": _refusing(G.image_load, self._handles(), path)["alive"]}

    def stamp(self, cells, x0, y0, op, strip=None):
        c = np.asarray(cells, dtype=bool)
        _refusing(self.b.stamp_bits, G.pattern_words_np(c), c.shape[1], c.shape[0], x0, y0, op)

    def step(self, n, want_flips=False):
        _refusing(self.b.step, n, want_flips)

    def step_flips(self, n, cap):
        import ctypes
        xy = np.zeros((max(cap, 1), 2), dtype=np.int32)
        counts = np.zeros(max(n, 1), dtype=np.uint64)
        tot = ctypes.c_uint64()
        rc = G.load().golhip_step_flips(self.b.handle, n, ctypes.c_void_p(xy.ctypes.data), cap,
                                        ctypes.c_void_p(counts.ctypes.data), ctypes.byref(tot))
        if rc not in (OK, ERANGE):
            raise Refused(rc)
        return (rc, xy[:min(cap, tot.value)], [int(c) for c in counts[:n]], tot.value)

    def flip_stream(self, n, cap, fmt, pinned=False):
        lib = G.load()
        return self._stream(lambda *a: lib.golhip_flip_stream(self.b.handle, *a), n, cap, fmt, pinned)

    def view_stream(self, n, every, view, cap_frames):
        x0, y0, s, ow, oh, fmt = view
        return _refusing(self.b.view_stream, n, every, x0, y0, s, ow, oh, fmt, cap_frames=cap_frames)

    def set_option(self, key, value):
        _refusing(self.b.set_option, key, value)

    def set_tb_depth(self, turns):
        _refusing(self.b.set_tb_depth, turns)

    def set_rows_per_wave(self, rows):
        _refusing(self.b.set_rows_per_wave, rows)

    def set_pad_step(self, mode):
        _refusing(self.b.set_pad_step, mode)

    def perf_reset(self):
        self.b.perf_reset()

    def perf(self):
        return self.b.perf()

    def turn(self):
        return self.b.turn()

    def alive_count(self):
        return self.b.alive_count()

    def board_hash(self):
        return self.b.board_hash()

    def snapshot_bytes(self):
        return self.b.snapshot_bytes()

    def snapshot_bits(self):
        return self.b.snapshot_bits()

    def snapshot_rows(self, row, nrows, strip=None):
        return self.b.snapshot_rows(row, nrows)

    def alive_cells(self):
        return self.b.alive_cells()

    def flips(self):
        return _refusing(self.b.flips)

    def view_frame(self, view):
        x0, y0, s, ow, oh, fmt = view
        return _refusing(self.b.view_frame, x0, y0, s, ow, oh, fmt)

    def checkpoint_begin(self, path):
        return self._begin(_refusing(G.checkpoint_begin, self._handles(), path))

    def image_begin(self, path):
        return self._begin(_refusing(G.image_begin, self._handles(), path))

    def set_rule(self, rule):
        _refusing(self.b.set_rule, tuple(rule))

    def stamp_file(self, path, x0, y0, op):
        return _refusing(G.stamp_file, self._handles(), path, x0, y0, op)

    def extract(self, x0, y0, w, h):
        return _refusing(self.b.extract, x0, y0, w, h)

    def alive_box(self):
        return _refusing(self.b.alive_box)

    def save_rle(self, path, box=None, chunk_rows=0):
        return _refusing(G.save_rle, self._handles(), path, box, chunk_rows)


class GroupTarget(_Target):
    """HandleModel's calls on the row strips [cuts[i], cuts[i + 1]) through the
    group entry points: rows concatenated, counts and digests summed, every
    strip's turn reported."""

    def __init__(self, W, H, cuts):
        self.W, self.H, self.cuts = W, H, list(cuts)
        self.bs = [G.Board(W, H, row0=a, rows=b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        self._init_jobs()

    def close(self):
        super().close()
        for b in self.bs:
            b.close()

    def _each(self, name, *a):
        for b in self.bs:
            _refusing(getattr(b, name), *a)

    def load_bytes(self, cells):
        for b in self.bs:
            _refusing(b.load_bytes, cells[b.row0:b.row0 + b.rows])

    def load_bits(self, words):
        for b in self.bs:
            _refusing(b.load_bits, words[b.row0:b.row0 + b.rows])

    def fill_random(self, seed):
        self._each("fill_random", seed)

    def clear(self):
        self._each("clear")

    def checkpoint_load(self, path):
        d = _refusing(G.checkpoint_load, self.bs, path)
        return {"turn": d["turn"], "alive": d["alive"]}

    def image_load(self, path):
        return {"alive": _refusing(G.image_load, self.bs, path)["alive"]}

    def stamp(self, cells, x0, y0, op, strip=None):
        c = np.asarray(cells, dtype=bool)
        if strip is None:
            _refusing(G.group_stamp, self.bs, c, x0, y0, op)
        else:
            _refusing(self.bs[strip].stamp_bits, G.pattern_words_np(c), c.shape[1], c.shape[0], x0, y0, op)

    def step(self, n, want_flips=False):
        _refusing(G.group_step, self.bs, n, want_flips)

    def flip_stream(self, n, cap, fmt, pinned=False):
        import ctypes
        lib = G.load()
        arr = (ctypes.c_void_p * len(self.bs))(*[b.handle for b in self.bs])
        return self._stream(lambda *a: lib.golhip_group_flip_stream(arr, len(self.bs), *a), n, cap, fmt, pinned)

    def view_stream(self, n, every, view, cap_frames):
        x0, y0, s, ow, oh, fmt = view
        return _refusing(G.group_view_stream, self.bs, n, every, x0, y0, s, ow, oh, fmt, cap_frames=cap_frames)

    def set_option(self, key, value):
        self._each("set_option", key, value)

    def set_tb_depth(self, turns):
        self._each("set_tb_depth", turns)

    def set_rows_per_wave(self, rows):
        self._each("set_rows_per_wave", rows)

    def set_pad_step(self, mode):
        _refusing(G.group_set_pad_step, self.bs, mode)

    def perf_reset(self):
        self._each("perf_reset")

    def perf(self):
        ps = [b.perf() for b in self.bs]
        out = {k: sum(p[k] for p in ps) for k in ps[0] if k not in ("kernel_variant", "words_per_lane")}
        out["kernel_variant"], out["words_per_lane"] = ps[0]["kernel_variant"], ps[0]["words_per_lane"]
        return out

    def turn(self):
        return tuple(b.turn() for b in self.bs)

    def alive_count(self):
        cs = [b.alive_count() for b in self.bs]
        return (sum(c for c, _ in cs), tuple(t for _, t in cs))

    def board_hash(self):
        return sum(b.board_hash() for b in self.bs) % 2 ** 64

    def snapshot_bytes(self):
        return np.concatenate([b.snapshot_bytes() for b in self.bs])

    def snapshot_bits(self):
        return np.concatenate([b.snapshot_bits() for b in self.bs])

    def snapshot_rows(self, row, nrows, strip=None):
        return self.bs[strip].snapshot_rows(row, nrows)

    def alive_cells(self):
        return np.concatenate([b.alive_cells() for b in self.bs])

    def flips(self):
        return np.concatenate([_refusing(b.flips) for b in self.bs])

    def view_frame(self, view):
        x0, y0, s, ow, oh, fmt = view
        return _refusing(G.group_view_frame, self.bs, x0, y0, s, ow, oh, fmt)

    def checkpoint_begin(self, path):
        return self._begin(_refusing(G.checkpoint_begin, self.bs, path))

    def image_begin(self, path):
        return self._begin(_refusing(G.image_begin, self.bs, path))

    def set_rule(self, rule):
        _refusing(G.group_set_rule, self.bs, tuple(rule))

    def stamp_file(self, path, x0, y0, op):
        return _refusing(G.stamp_file, self.bs, path, x0, y0, op)

    def extract(self, x0, y0, w, h):
        return _refusing(G.group_extract, self.bs, x0, y0, w, h)

    def alive_box(self):
        return _refusing(G.group_alive_box, self.bs)

    def save_rle(self, path, box=None, chunk_rows=0):
        return _refusing(G.save_rle, self.bs, path, box, chunk_rows)

    def split_rule(self, strip, rule, what, args):
        old = self.bs[strip].rule()
        _refusing(self.bs[strip].set_rule, tuple(rule))
        try:
            code = replay(self, what, *args)
        finally:
            _refusing(self.bs[strip].set_rule, old)
        path = args[0] if what == "save_rle" else None
        wrote = path is not None and (os.path.exists(path) or os.path.exists(path + ".tmp"))
        return (OK if code[0] == "ok" else code[1], wrote)


# --------------------------------------------------------------------------- the tables
# (weight, kind).  A kind is a generator below: gen_<kind>(driver) -> (method, args, kwargs, pre).
MUTATING = {"load_bytes", "load_bits", "fill_random", "clear", "checkpoint_load", "image_load", "stamp", "step",
            "step_flips", "flip_stream", "view_stream", "stamp_file", "split_rule"}
STEPPING = {"step", "step_flips", "flip_stream", "view_stream"}
REPLACING = {"load_bytes", "load_bits", "fill_random", "clear", "checkpoint_load", "image_load", "wpl"}

TORUS_TABLE = [
    (3, "load_bytes"), (3, "load_bits"), (3, "fill_random"), (3, "clear"), (3, "checkpoint_load"), (2, "image_load"),
    (14, "stamp"), (12, "step"), (5, "step_flips"), (9, "flip_stream"), (4, "view_stream"),
    (6, "set_wpl"), (3, "set_persistent"), (3, "set_lds_band"), (3, "set_skew"), (2, "set_timing"),
    (3, "set_flip_overlap"), (4, "set_tb_depth"), (2, "set_rows_per_wave"), (3, "set_pad_step"), (2, "perf_reset"),
    (2, "alive_cells"), (2, "snapshot"), (9, "flips"), (3, "view_frame"),
    (5, "checkpoint_begin"), (4, "image_begin"),
    # calls the header refuses: 12 of 141 by weight (the first load and the prefixes are never refused);
    # the ERANGE draws of the streams and flips() without a list come on top
    (6, "refused_stamp"), (3, "refused_option"), (3, "refused_view_stream"),
]
# (golhip_step_flips has no group entry point; "persistent" and "lds_band" are accepted on strips and change nothing)
GROUP_TABLE = [(w, k) for w, k in TORUS_TABLE if k != "step_flips"] + [(6, "stamp_strip")]

# The tables of the "-rules" configurations: the old ones (left as they are: adding a kind
# changes every draw of the sequences already committed) and the calls of the Life-like
# rules and of the pattern savers.  Refused by the header: 12 + 4 of 167 by weight, and
# the stamp_file draws whose file names another rule than the handle's.
RULE_KINDS = [(12, "set_rule"), (5, "extract"), (3, "alive_box"), (6, "save_rle"), (8, "stamp_file"),
              (2, "refused_set_rule"), (2, "refused_extract")]
TORUS_RULES_TABLE = TORUS_TABLE + RULE_KINDS
GROUP_RULES_TABLE = GROUP_TABLE + RULE_KINDS + [(12, "split_rule")]  # (seven group calls to draw from)
TABLES = {None: (TORUS_TABLE, GROUP_TABLE), "rules": (TORUS_RULES_TABLE, GROUP_RULES_TABLE)}

# what gen_set_rule draws: Conway's often enough that its kernel families still occur
RULE_DRAWS = [CONWAY] * 4 + list(STATIC_RULES.values()) + list(DYNAMIC_RULES.values())
HAND_RLES = ["x = 3, y = 3\nbo$2bo$3o!\n", "#C a glider\nx = 3, y = 3\nbo$\n2bo$ 3o !\n", "x = 4, y = 2\n4o$o2bo!\n",
             "x = 5, y = 3\n!\n"]


def table_kinds(table) -> list[str]:
    return [k for _, k in table]


class Driver:
    """One sequence: draws calls, applies each to the model and the target, compares."""

    def __init__(self, target, model, rng, table, tmpdir, stats=None, name="t"):
        self.target, self.model, self.rng, self.table, self.tmp = target, model, rng, table, str(tmpdir)
        self.stats = stats if stats is not None else {}
        self.name = name
        self.lines: list[str] = []
        self.files: list[str] = []     # checkpoint files a finished job of this sequence wrote
        self.pending: list[list] = []  # [job, calls left before the wait, kinds seen since begin]
        self.nfile = 0
        self.depth = 20                # the handle's tb_depth (its default)
        self.last_perf = None
        self.last_wpl = None
        self.lds_band = -1             # option "lds_band" as last accepted (its default: automatic)
        self.rles: list[str] = []      # RLE files a save_rle of this sequence wrote
        self.rules = any(k == "set_rule" for _, k in table)  # the "-rules" tables: their extra checks
        self.since_wpl: set = set()    # accepted calls since words_per_lane was last read
        self.rule_at_wpl = CONWAY
        w = np.array([x for x, _ in table], dtype=float)
        self.weights = w / w.sum()
        for key, zero in (("kinds", {}), ("families", set()), ("wpl_moves", set()), ("jobs_between", []), ("notes", set()),
                          ("rules_stepped", set()), ("rule_wpl_moves", set()), ("trail", [])):
            self.stats.setdefault(key, zero)

    # ---- drawing
    def pick(self, xs):
        return xs[int(self.rng.integers(len(xs)))]

    def seed(self) -> int:
        return int(self.rng.integers(1, 2 ** 31))

    def path(self, ext) -> str:
        self.nfile += 1
        return os.path.join(self.tmp, f"{self.name}_{self.nfile}.{ext}")

    def board_cells(self) -> Cells:
        return Cells("board", self.model.W, self.model.H, self.seed(), self.pick([0, 0, 1, 2]))

    def pattern(self):
        """A pattern and its corner, biased to the x seam, the y seam and the 32 / 64 / 128-cell boundaries."""
        W, H = self.model.W, self.model.H
        pw = self.pick([w for w in (1, 31, 32, 33, W - 1, W) if 1 <= w <= W])
        ph = self.pick([h for h in (1, 2, 5, H - 1, H) if 1 <= h <= H])
        edges = [e for e in (32, 64, 128) if e < W]
        mode = self.pick(["seam", "edge", "any"])
        if mode == "seam":
            x0 = (W - int(self.rng.integers(1, max(2, min(pw, W)))) % W) % W
        elif mode == "edge" and edges:
            x0 = max(0, min(W - 1, self.pick(edges) - int(self.rng.integers(0, max(1, min(pw, 33))))))
        else:
            x0 = int(self.rng.integers(W))
        y0 = (H - 1 - int(self.rng.integers(0, max(1, min(ph, H))))) % H if self.rng.random() < 0.5 \
            else int(self.rng.integers(H))
        return Cells("pattern", pw, ph, self.seed()), x0, y0

    def view(self, scale1=False):
        W, H = self.model.W, self.model.H
        s = 1 if scale1 else self.pick([s for s in (1, 1, 2, 3, 5) if s <= min(W, H)])
        ow, oh = int(self.rng.integers(1, W // s + 1)), int(self.rng.integers(1, H // s + 1))
        if self.rng.random() < 0.3:
            ow, oh = W // s, H // s
        return (int(self.rng.integers(W)), int(self.rng.integers(H)), s, ow, oh, self.pick([G.VIEW_ARGB, G.VIEW_GRAY8]))

    def turns(self) -> int:
        d = self.depth
        return self.pick([0, 1, d - 1, d, d + 1, 2 * d + 5, 1, 2, 3])

    # ---- the kinds: (method, args, kwargs, pre)
    def gen_load_bytes(self):
        return "load_bytes", (self.board_cells(),), {}, []

    def gen_load_bits(self):
        m = self.model
        return "load_bits", (Cells("words", m.W, m.H, self.seed(), self.pick([0, 1]), 1),), {}, []

    def gen_fill_random(self):
        return "fill_random", (self.seed(),), {}, []

    def gen_clear(self):
        return "clear", (), {}, []

    def gen_checkpoint_load(self):
        if self.files and self.rng.random() < 0.6:
            return "checkpoint_load", (self.pick(self.files),), {}, []
        p = self.path("ckpt")
        return "checkpoint_load", (p,), {}, [("write_ckpt", (p, self.board_cells(), int(self.rng.integers(0, 1000))))]

    def gen_image_load(self):
        p = self.path("pgm")
        return "image_load", (p,), {}, [("write_pgm", (p, self.board_cells()))]

    def gen_stamp(self):
        c, x0, y0 = self.pattern()
        return "stamp", (c, x0, y0, self.pick([0, 1, 2, 3])), {}, []

    def gen_stamp_strip(self):
        c, x0, y0 = self.pattern()
        return "stamp", (c, x0, y0, self.pick([0, 1, 2, 3])), {"strip": int(self.rng.integers(self.model.nstrips))}, []

    def gen_step(self):
        return "step", (self.turns(), bool(self.rng.random() < 0.5)), {}, []

    def _list_sizes(self, n):
        return [len(l) for _, l in self.model._lists(n)]

    def gen_step_flips(self):
        n = self.pick([0, 1, 2, 3, 5])
        sizes = self._list_sizes(n)
        cap = sum(sizes) if self.rng.random() < 0.6 else max(0, sum(sizes) - 1 - int(self.rng.integers(0, 1 + sum(sizes) // 2)))
        return "step_flips", (n, cap), {}, []

    def gen_flip_stream(self):
        n = self.pick([0, 1, 2, 3, 4, 6])
        sizes = self._list_sizes(n)
        how = self.pick(["ample", "ample", "exact", "stops", "stops", "small"])
        if how == "ample" or not sizes:
            cap = min(max(1, n) * self.model.W * self.model.H, 4 * sum(sizes) + 64)
        elif how == "exact":
            cap = sum(sizes)
        elif how == "stops":  # the first k lists and part of the next
            k = int(self.rng.integers(1, max(2, len(sizes))))
            cap = sum(sizes[:k]) + (sizes[k] // 2 if k < len(sizes) else 0)
            cap = max(cap, sizes[0])
        else:
            cap = max(0, sizes[0] - 1)  # under the first turn's list (or a first list that is empty: cap 0 fits)
        return "flip_stream", (n, cap, self.pick([G.FLIPS_XY, G.FLIPS_INDEX])), {"pinned": bool(self.rng.random() < 0.5)}, []

    def gen_view_stream(self):
        n, every = self.pick([0, 1, 3, 4, 7]), self.pick([1, 2, 3])
        return "view_stream", (n, every, self.view(), n // every), {}, []

    def gen_set_wpl(self):
        return "set_option", ("wpl", self.pick([0, 1, 2, 4])), {}, []

    def gen_set_persistent(self):
        return "set_option", ("persistent", self.pick([-1, 0, 1, 1])), {}, []

    def gen_set_lds_band(self):
        return "set_option", ("lds_band", self.pick([-1, 0, 1])), {}, []

    def gen_set_skew(self):
        return "set_option", ("skew", self.pick([0, 1, 2, 2])), {}, []

    def gen_set_timing(self):
        return "set_option", ("timing", self.pick([0, 1])), {}, []

    def gen_set_flip_overlap(self):
        return "set_option", ("flip_overlap", self.pick([0, 1, 2, 3, 3])), {}, []

    def gen_set_tb_depth(self):
        return "set_tb_depth", (self.pick([32, 24, 20, 18, 16, 12, 9, 8, 6, 4, 2, 1, 3, 5, 7]),), {}, []

    def gen_set_rows_per_wave(self):
        return "set_rows_per_wave", (self.pick([0, 1, 2, 5, 37]),), {}, []

    def gen_set_pad_step(self):
        return "set_pad_step", (self.pick([-1, 0, 1, 1]),), {}, []

    def gen_perf_reset(self):
        return "perf_reset", (), {}, []

    def gen_alive_cells(self):
        return "alive_cells", (), {}, []

    def gen_snapshot(self):
        return self.pick(["snapshot_bytes", "snapshot_bits"]), (), {}, []

    def gen_flips(self):
        if self.model.flip == UNKNOWN:  # the header is silent here: ask for something it does define
            return "alive_cells", (), {}, []
        return "flips", (), {}, []

    def gen_view_frame(self):
        return "view_frame", (self.view(),), {}, []

    def gen_checkpoint_begin(self):
        return "checkpoint_begin", (self.path("ckpt"),), {}, []

    def gen_image_begin(self):
        return "image_begin", (self.path("pgm"),), {}, []

    def gen_refused_stamp(self):
        W, H = self.model.W, self.model.H
        c, x0, y0 = self.pattern()
        how = self.pick(["off_x", "off_y", "wide", "tall", "op"])
        if how == "off_x":
            return "stamp", (c, self.pick([W, -1]), y0, 1), {}, []
        if how == "off_y":
            return "stamp", (c, x0, self.pick([H, -1]), 1), {}, []
        if how == "wide":
            return "stamp", (Cells("pattern", W + 1, 1, self.seed()), x0, y0, 1), {}, []
        if how == "tall":
            return "stamp", (Cells("pattern", 1, H + 1, self.seed()), x0, y0, 1), {}, []
        return "stamp", (c, x0, y0, 4), {}, []

    def gen_refused_option(self):
        return self.pick([("set_option", ("wpl", 3), {}, []), ("set_tb_depth", (0,), {}, []),
                          ("set_tb_depth", (33,), {}, []), ("set_option", ("skew", 3), {}, []),
                          ("set_pad_step", (2,), {}, [])])

    def gen_refused_view_stream(self):
        every = self.pick([1, 2])
        n = every * self.pick([2, 3])
        return "view_stream", (n, every, self.view(), n // every - 1), {}, []

    # ---- the kinds of the "-rules" tables
    def rect(self):
        """A rectangle biased as pattern() biases stamps; on a group half of those taller than a row span a cut."""
        c, x0, y0 = self.pattern()
        pw, ph = c.a[0], c.a[1]
        m = self.model
        if m.cuts is not None and ph > 1 and self.rng.random() < 0.5:
            y0 = (self.pick(m.cuts[1:-1]) - int(self.rng.integers(1, ph))) % m.H
        return x0, y0, pw, ph

    def other_rule(self):
        return self.pick([r for r in RULE_DRAWS if r != self.model.rule])

    def gen_set_rule(self):
        return "set_rule", (self.pick(RULE_DRAWS),), {}, []

    def gen_extract(self):
        return "extract", self.rect(), {}, []

    def gen_alive_box(self):
        return "alive_box", (), {}, []

    def gen_save_rle(self):
        box = None if self.rng.random() < 0.5 else self.rect()
        return "save_rle", (self.path("rle"), box, self.pick([0, 1, 2, 7])), {}, []

    def gen_stamp_file(self):
        c, x0, y0 = self.pattern()
        op = self.pick([0, 1, 2, 3])
        how = self.pick(["saved", "saved", "written", "written", "hand"])
        if how == "saved" and self.rles:  # a file of this sequence: its rule may or may not be today's
            return "stamp_file", (self.pick(self.rles), x0, y0, op), {}, []
        p = self.path("rle")
        if how == "hand":  # names no rule: every handle takes it
            return "stamp_file", (p, x0, y0, op), {}, [("write_text", (p, self.pick(HAND_RLES)))]
        rule = self.model.rule if self.rng.random() < 0.5 else self.pick(RULE_DRAWS)
        return "stamp_file", (p, x0, y0, op), {}, [("write_rle", (p, c, rule))]

    def gen_refused_set_rule(self):
        b, s = self.pick(RULE_DRAWS)
        return "set_rule", (self.pick([(b | 0x200, s), (b, s | 0x200), (0x200, 0x200)]),), {}, []

    def gen_refused_extract(self):
        W, H = self.model.W, self.model.H
        x0, y0, w, h = self.rect()
        return "extract", self.pick([(W, y0, w, h), (x0, H, w, h), (-1, y0, w, h), (x0, y0, W + 1, h),
                                     (x0, y0, w, H + 1), (x0, y0, 0, h), (x0, y0, w, 0)]), {}, []

    def gen_split_rule(self):
        """One strip on another rule, one group call (refused: EINVAL), the strip set back."""
        m = self.model
        what = self.pick(["step", "flip_stream", "view_frame", "stamp", "extract", "alive_box", "save_rle"])
        if what == "step":
            args = (self.pick([1, 2, self.depth + 1]),)
        elif what == "flip_stream":
            args = (self.pick([1, 3]), m.W * m.H, G.FLIPS_XY)
        elif what == "view_frame":
            args = (self.view(),)
        elif what == "stamp":
            c, x0, y0 = self.pattern()
            args = (c, x0, y0, self.pick([0, 1, 2, 3]))
        elif what == "extract":
            args = self.rect()
        elif what == "alive_box":
            args = ()
        else:
            args = (self.path("rle"), self.pick([None, self.rect()]), 0)
        return "split_rule", (int(self.rng.integers(m.nstrips)), self.other_rule(), what, args), {}, []

    def saved(self, args, got):
        """The file of a save_rle: its cells, its rule, its #CXRLE line; or no file at all."""
        path, box, _ = args
        m = self.model
        if got[0] != "ok":
            if os.path.exists(path) or os.path.exists(path + ".tmp"):
                self.fail(f"save_rle: refused with {got[1]} and left {path} or its .tmp")
            if box is None and not _alive(m.board):
                self.stats["notes"].add("save_rle_empty")
            return
        box = box if box is not None else tuple(int(v) for v in G.alive_box_np(m.board))
        with open(path) as f:
            text = f.read()
        named, bare = rle_split(text)
        if os.path.exists(path + ".tmp"):
            self.fail(f"save_rle: {path}.tmp is left")
        if text.split("\n")[0] != f"#CXRLE Pos={box[0]},{box[1]} Gen={m.t}":
            self.fail(f"save_rle: {path} begins {text[:60]!r}, the box is {box} and the turn {m.t}")
        if named != m.rule or tuple(G.pattern_rule(path)) != m.rule:
            self.fail(f"save_rle: {path} names the rule {named}, the handle has {m.rule}")
        if not np.array_equal(G.rle_parse_np(bare), G.extract_np(m.board, *box)):
            self.fail(f"save_rle: the cells of {path} are not the board's at {box}")
        self.rles.append(path)

    # ---- applying
    def fail(self, what, got=None):
        m = self.model
        make = f"hm.BoardTarget({m.W}, {m.H})" if m.cuts is None else f"hm.GroupTarget({m.W}, {m.H}, {m.cuts})"
        head = [f"# {what}"[:300], "import oracle.handle_model as hm", f"{self.name} = {make}"]
        e = SequenceMismatch(f"{what}\n" + "\n".join(head + self.lines))
        e.lines, e.got = head + self.lines, got
        raise e

    @staticmethod
    def same(a, b) -> bool:
        if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
            a, b = np.asarray(a), np.asarray(b)
            return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))
        if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
            return len(a) == len(b) and all(Driver.same(x, y) for x, y in zip(a, b))
        if isinstance(a, dict) and isinstance(b, dict):
            return a.keys() == b.keys() and all(Driver.same(a[k], b[k]) for k in a)
        return a == b

    def call(self, method, args=(), kwargs=None, pre=()):
        """One call on the target, then on the model; their answers must agree."""
        kwargs = dict(kwargs or {})
        for fn, a in pre:
            self.lines.append(f"hm.{fn}({', '.join(map(repr, a))})")
            globals()[fn](*a)
        tail = "".join([f", {a!r}" for a in args] + [f", {k}={v!r}" for k, v in kwargs.items()])
        self.lines.append(f"hm.replay({self.name}, {method!r}{tail})")
        raw = got = replay(self.target, method, *args, **kwargs)
        mk = dict(kwargs)
        if method == "flip_stream" and got[0] == "ok":
            mk["done"] = got[1][2]
        try:
            want = replay(self.model, method, *args, **mk)
        except SequenceMismatch as e:
            self.fail(f"{method}: {e}", raw)
        if got[0] == "refused" and want[0] == "refused" and (got[2] is None or want[2] is None):
            got, want = got[:2], want[:2]  # (only the flip streams report what they need)
        if method in ("checkpoint_begin", "image_begin") and got[0] == want[0] == "ok":
            return got[1], want[1]
        if not self.same(got, want):
            self.fail(f"{method}: the target answered {self._short(got)}, the model {self._short(want)}", raw)
        return got, want

    @staticmethod
    def _short(x):
        s = repr(x)
        return s if len(s) < 400 else s[:400] + " ..."

    def cheap(self):
        for m in ("turn", "alive_count", "board_hash"):
            self.call(m)
        if self.model.flip != UNKNOWN and self.rng.random() < 0.5:  # the list, or EINVAL, as the model says
            self.call("flips")
        if self.rules:
            self.call("alive_box")

    def full(self):
        m = self.model
        for name in ("snapshot_bytes", "snapshot_bits", "alive_cells"):
            self.call(name)
        strip = None if m.cuts is None else int(self.rng.integers(m.nstrips))
        rows = m.H if strip is None else m.cuts[strip + 1] - m.cuts[strip]
        r = int(self.rng.integers(rows))
        self.call("snapshot_rows", (r, int(self.rng.integers(0, rows - r + 1))), {} if strip is None else {"strip": strip})
        self.call("view_frame", ((0, 0, 1, m.W, m.H, G.VIEW_GRAY8),))
        if self.rules:  # one drawn extract, and what an observer promises to leave: the kept count and the flip list
            self.call("extract", self.rect())
            self.call("alive_count")
            if m.flip != UNKNOWN:
                self.call("flips")

    def classify(self, method):
        """The kernel families a stepping call took, from the change in perf()."""
        p = self.target.perf()
        if p is None:
            return
        q = self.last_perf if self.last_perf is not None else {k: 0 for k in p}
        d = {k: p[k] - q.get(k, 0) for k in p if isinstance(p[k], int)}
        self.last_perf = p
        if method == "perf_reset":
            return
        if method not in STEPPING:
            return
        fam, W = self.stats["families"], self.model.W
        if d["pad_launches"] > 0:
            fam.add("padded")
        if d["lds_launches"] > 0:
            fam.add("K1r")
        if d["persist_launches"] - d["lds_launches"] > 0:
            fam.add("K1p")
        if d["persist_fallbacks"] > 0 and self.lds_band >= 0:
            # a resident launch that fell back on a shared GPU: an attempt on the family the
            # sequence asked for ("lds_band" 1: K1r, 0: K1p; left automatic it names neither)
            fam.add("K1r" if self.lds_band == 1 else "K1p")
        if d["pair_launches"] > 0:
            fam.add("K1w-pair")
        if d["skew_launches"] - d["pair_launches"] > 0:
            fam.add("K1w")
        if d["step_launches"] - d["skew_launches"] > 0 and d["pad_launches"] == 0:
            # per-launch kernels besides K1w: kernel_variant names the last launch's
            # (0 the any-width kernel, words_per_lane 0; 1 bit-sliced; a K1w launch last names neither)
            if p["kernel_variant"] == 0 and p["words_per_lane"] == 0:
                fam.add("K1g")
            elif p["kernel_variant"] == 1 and p["words_per_lane"] in (1, 2, 4):
                fam.add("K1")
        if d["flip_launches"] > 0:
            fam.add("K5")
        if d["flip_resident_launches"] > 0:
            fam.add("K5r")
        rule = self.model.rule
        if d["rule_launches"] > 0:  # the rule kernel K11: canonical words, any width
            self.stats["rules_stepped"].add(rule)
            if d["pad_launches"] > 0:
                fam.add("K11-padded")
            elif W % 32:
                fam.add("K11-seam")
            else:
                fam.add("K11-static" if rule in STATIC_RULES.values() else "K11-dynamic")
            if method in ("flip_stream", "step_flips") and d["flip_launches"] == 0 and d["flip_resident_launches"] == 0:
                fam.add("K11-flips")
        if d["rule_launches"] > 0:  # which kind of kernel each stepping call of the sequence ran on
            self.stats["trail"].append("K11")
        elif d["step_launches"] + d["persist_launches"] + d["flip_launches"] + d["flip_resident_launches"] > 0:
            self.stats["trail"].append("Conway")
        if method in ("step", "view_stream") and W % 32 == 0 and d["step_turns"] + d["persist_turns"] > 0:
            wpl = p["words_per_lane"]
            if self.last_wpl is not None and wpl != self.last_wpl:
                self.stats["wpl_moves"].add((self.last_wpl, wpl))
                # a move that a set_rule made: the board was not replaced and option "wpl" not set in between
                if rule != self.rule_at_wpl and "set_rule" in self.since_wpl and not self.since_wpl & REPLACING:
                    self.stats["rule_wpl_moves"].add((self.last_wpl, wpl))
            self.last_wpl, self.rule_at_wpl, self.since_wpl = wpl, rule, set()

    def finish_job(self, entry):
        job_t, job_m = entry[0]
        kind, path, board, turn = self.model.job_expect(job_m)
        self.lines.append(f"hm.replay({self.name}, 'wait', {job_t})  # {path}")
        got = replay(self.target, "wait", job_t)
        want = replay(self.model, "wait", job_m)
        if got != want:
            self.fail(f"wait: the target reported {got}, the model {want}", got)
        if kind == "ckpt":
            info, words = G.checkpoint_read_np(path)
            ok = info["turn"] == turn and np.array_equal(words, pack_bits(board))
            self.files.append(path)
        else:
            ok = np.array_equal(read_pgm(path, self.model.W, self.model.H), board)
        if not ok:
            self.fail(f"wait: {path} does not hold the board and turn of its begin (turn {turn})")
        self.stats["jobs_between"].append(frozenset(entry[2]))

    def run(self, n_ops, prefix=()):
        """A load first (a handle never loaded is outside the tables), the
        prefix, then drawn calls up to n_ops in all."""
        kinds = table_kinds(self.table)
        todo = [("fill_random", self.gen_fill_random())] + [(None, p) for p in prefix]
        for i in range(n_ops):
            if i < len(todo):
                kind, (method, args, kwargs, pre) = todo[i]
            else:
                kind = kinds[int(self.rng.choice(len(kinds), p=self.weights))]
                method, args, kwargs, pre = getattr(self, "gen_" + kind)()
            if kind is not None:
                self.stats["kinds"][kind] = self.stats["kinds"].get(kind, 0) + 1
            t_before = self.model.t
            got, want = self.call(method, args, kwargs, pre)
            if method == "save_rle":
                self.saved(args, got)
            if method == "split_rule":
                self.stats["notes"].add("split_rule:" + args[2])
            if method == "stamp_file":
                with open(args[0]) as f:
                    named = rle_split(f.read())[0]
                if got[0] == "ok":
                    self.stats["notes"].add("stamp_file_accepted")
                    if args[0] in self.rles:  # the writer's own header back through the library's parser
                        self.stats["notes"].add("stamp_file_saved_accepted")
                elif named is not None and named != self.model.rule:
                    self.stats["notes"].add("stamp_file_refused_for_its_rule")
            if isinstance(got, tuple) and got[0] == "ok":
                self.since_wpl.add(args[0] if method == "set_option" else method)
            if method in ("checkpoint_begin", "image_begin"):
                self.pending.append([(got, want), int(self.rng.integers(1, 7)), set()])
            else:
                if method == "set_tb_depth" and got[0] == "ok":
                    self.depth = args[0]
                if method == "set_option" and got[0] == "ok" and args[0] == "lds_band":
                    self.lds_band = args[1]
                word = "step" if method in STEPPING and self.model.t != t_before else method
                for e in self.pending:
                    if got[0] == "ok":  # (a refused call changed nothing: it is no stamp, clear or step)
                        e[2].add(word)
                    e[1] -= 1
            if method in MUTATING:
                self.cheap()
            self.classify(method)
            for e in [e for e in self.pending if e[1] <= 0]:
                self.pending.remove(e)
                self.finish_job(e)
            if i % 8 == 7:
                self.full()
        for e in list(self.pending):
            self.pending.remove(e)
            self.finish_job(e)
        self.cheap()
        self.full()


def run_sequence(target, model, rng, n_ops, table, tmpdir, stats=None, prefix=(), name="t"):
    """n_ops calls drawn from `table` with `rng` (numpy.random.default_rng(seed)),
    each applied to `target` and to `model`.  After every mutating call turn(),
    alive_count() and board_hash() are compared; after every eighth call and at
    the end snapshot_bytes, snapshot_bits, snapshot_rows of a random interval,
    alive_cells and view_frame at scale 1 -- all by exact equality.  Raises
    SequenceMismatch with the calls so far as Python lines.  A table with the
    kind "set_rule" (the "-rules" tables) adds alive_box() after every mutating
    call and, after every eighth, one drawn extract with alive_count() and
    flips() behind it; the first tables' sequences draw and compare what they
    always did (tests/golden/sequence_lines_parent.json pins their lines).
    `stats` collects the call kinds drawn, the kernel families taken (from
    perf()), the moves of words_per_lane (and those a set_rule made), the rules
    that stepped on K11, whether each stepping call ran on K11 or on a Conway
    kernel, notes for the CPU coverage condition and what fell between each
    job's begin and wait."""
    d = Driver(target, model, rng, table, tmpdir, stats, name)
    d.run(n_ops, prefix)
    return d


# --------------------------------------------------------------------------- the committed configurations
# The boards are the smallest at which each path exists (tests/test_gpu_sequences.py
# says what only each reaches); `prefix` calls follow the first load.  The seeds
# are literals in the two test files.
CONFIGS = {
    "128x17": dict(W=128, H=17, prefix=[("set_option", ("persistent", 1), {}, [])]),
    "256x40": dict(W=256, H=40, prefix=[("set_option", ("persistent", 1), {}, []), ("set_option", ("wpl", 4), {}, [])]),
    "192x33": dict(W=192, H=33, prefix=[("set_option", ("persistent", 0), {}, [])]),
    "96x20": dict(W=96, H=20, prefix=[("set_option", ("skew", 2), {}, [])]),
    "100x37": dict(W=100, H=37),
    "33x9": dict(W=33, H=9),
    "5x3": dict(W=5, H=3),
    # K1w needs rows for a stack of bands: 123 for the pair rule's 18 turns at two words per lane
    "128x130": dict(W=128, H=130, prefix=[("set_option", ("skew", 2), {}, []), ("set_option", ("persistent", 0), {}, []),
                                          ("set_option", ("wpl", 2), {}, []), ("step", (41, False), {}, []),
                                          ("set_tb_depth", (16,), {}, []), ("step", (33, True), {}, [])]),
    "128x50-strips": dict(W=128, H=50, cuts=[0, 7, 17, 50]),
    "100x50-strips": dict(W=100, H=50, cuts=[0, 7, 17, 50]),
    # the "-rules" tables (set_rule, the pattern savers) on the boards above
    "128x17-rules": dict(W=128, H=17, table="rules", prefix=[("set_option", ("persistent", 1), {}, [])]),
    "192x33-rules": dict(W=192, H=33, table="rules", prefix=[("set_option", ("persistent", 0), {}, [])]),
    "100x37-rules": dict(W=100, H=37, table="rules"),
    "33x9-rules": dict(W=33, H=9, table="rules"),
    "128x130-rules": dict(W=128, H=130, table="rules",
                          prefix=[("set_option", ("skew", 2), {}, []), ("set_option", ("persistent", 0), {}, []),
                                  ("set_option", ("wpl", 2), {}, []), ("step", (41, False), {}, []),
                                  ("set_tb_depth", (16,), {}, []), ("step", (33, True), {}, [])]),
    "128x50-strips-rules": dict(W=128, H=50, table="rules", cuts=[0, 7, 17, 50]),
    "100x50-strips-rules": dict(W=100, H=50, table="rules", cuts=[0, 7, 17, 50]),
}


def config_table(name):
    """The table a committed configuration draws from: by its key "table", a torus' or a group's."""
    c = CONFIGS[name]
    return TABLES[c.get("table")][1 if c.get("cuts") else 0]


def run_config(name, seed, tmpdir, target=None, stats=None, n_ops=40, **model_args):
    """One committed sequence: configuration `name`, seed `seed`, against
    `target` (None: a BoardTarget / GroupTarget on the GPU)."""
    c = CONFIGS[name]
    cuts = c.get("cuts")
    model = HandleModel(c["W"], c["H"], cuts, **model_args)
    own = target is None
    if own:
        target = BoardTarget(c["W"], c["H"]) if cuts is None else GroupTarget(c["W"], c["H"], cuts)
    try:
        return run_sequence(target, model, np.random.default_rng(seed), n_ops, config_table(name),
                            tmpdir, stats, c.get("prefix", ()), name="t")
    finally:
        if own:
            target.close()
