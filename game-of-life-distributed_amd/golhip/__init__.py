"""ctypes binding of libgolhip.so (include/golhip.h).

This is plumbing for tests, the bench and the host mirror: every call goes
straight to the HIP library.  There is no CPU fallback — if libgolhip.so is
missing or no HIP device is present, construction raises.
"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GOLHIP_LIB") or os.path.join(HERE, "libgolhip.so")  # override: A/B builds
HEADER = os.path.join(HERE, "..", "..", "include", "golhip.h")

GOLHIP_OK = 0
GOLHIP_EINVAL = -1
GOLHIP_ERANGE = -4
GOLHIP_ECORRUPT = -6
FLIPS_XY, FLIPS_INDEX = 0, 1
FLAG_TIMING = 0x1
UNIQUE_ID_BYTES = 128
MAX_TB_DEPTH = 32
HALO_ROWS = 128  # GOLHIP_HALO_ROWS
VIEW_ARGB, VIEW_GRAY8 = 0, 1  # GOLHIP_VIEW_ARGB8888, GOLHIP_VIEW_GRAY8
VIEW_MAX_SCALE = 1024
STAMP_COPY, STAMP_OR, STAMP_XOR, STAMP_CLEAR = 0, 1, 2, 3  # GOLHIP_STAMP_*


class GolHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"golhip error {code}: {msg}")
        self.code = code


class Perf(ctypes.Structure):
    _fields_ = [
        ("turns", ctypes.c_int64),
        ("step_launches", ctypes.c_int64),
        ("step_turns", ctypes.c_int64),
        ("step_kernel_ms", ctypes.c_double),
        ("persist_launches", ctypes.c_int64),
        ("persist_turns", ctypes.c_int64),
        ("persist_kernel_ms", ctypes.c_double),
        ("cell_updates", ctypes.c_int64),
        ("alg_bytes", ctypes.c_int64),
        ("halo_bytes", ctypes.c_int64),
        ("tb_depth", ctypes.c_int32),
        ("rows_per_wave", ctypes.c_int32),
        ("kernel_variant", ctypes.c_int32),
        ("words_per_lane", ctypes.c_int32),
        ("persist_fallbacks", ctypes.c_int64),
        ("flip_launches", ctypes.c_int64),
        ("flip_entries", ctypes.c_int64),
        ("flip_kernel_ms", ctypes.c_double),
        ("flip_fallbacks", ctypes.c_int64),
        ("persist_depth", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("pad_launches", ctypes.c_int64),
        ("skew_launches", ctypes.c_int64),
        ("halo_exchanges", ctypes.c_int64),
        ("halo_ms", ctypes.c_double),
        ("rule_launches", ctypes.c_int64),
        ("skew_half_launches", ctypes.c_int64),
        ("lds_launches", ctypes.c_int64),
        ("pair_launches", ctypes.c_int64),
        ("pair_turns", ctypes.c_int64),
        ("flip_resident_launches", ctypes.c_int64),
        ("view_frames", ctypes.c_int64),
        ("view_kernel_ms", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class HaloPlan(ctypes.Structure):
    _fields_ = [
        ("prev_rank", ctypes.c_int32), ("next_rank", ctypes.c_int32),
        ("send_up_row", ctypes.c_int32), ("recv_top_row", ctypes.c_int32),
        ("send_down_row", ctypes.c_int32), ("recv_bottom_row", ctypes.c_int32),
        ("rows", ctypes.c_int32), ("bytes", ctypes.c_int64),
    ]


class View(ctypes.Structure):
    """golhip_view_t"""
    _fields_ = [
        ("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("scale", ctypes.c_int32),
        ("out_w", ctypes.c_int32), ("out_h", ctypes.c_int32), ("format", ctypes.c_int32),
    ]


class CkptOpts(ctypes.Structure):
    """golhip_ckpt_opts_t"""
    _fields_ = [("chunk_rows", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class CkptInfo(ctypes.Structure):
    """golhip_ckpt_info_t"""
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("turn", ctypes.c_int64),
        ("alive", ctypes.c_uint64), ("hash", ctypes.c_uint64), ("file_bytes", ctypes.c_uint64),
        ("stall_ms", ctypes.c_double), ("drain_ms", ctypes.c_double), ("write_ms", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class ImageInfo(ctypes.Structure):
    """golhip_image_info_t"""
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("turn", ctypes.c_int64),
        ("alive", ctypes.c_uint64), ("file_bytes", ctypes.c_uint64),
        ("header_bytes", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
        ("stall_ms", ctypes.c_double), ("drain_ms", ctypes.c_double), ("write_ms", ctypes.c_double),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class PatternInfo(ctypes.Structure):
    """golhip_pattern_info_t"""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("alive", ctypes.c_uint64),
                ("format", ctypes.c_int32), ("reserved", ctypes.c_int32)]

    def as_dict(self) -> dict:
        return {"width": self.width, "height": self.height, "alive": self.alive,
                "format": "pgm" if self.format == 1 else "rle"}


_lib = None

# golhip_test_transport_fn (test hook): user, prev_rank, next_rank, send_up,
# send_down, recv_top, recv_bottom, bytes -> 0
TRANSPORT_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)


def header_symbols(path: str = HEADER) -> list[str]:
    """Every function declared in include/golhip.h."""
    with open(path) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(golhip_[a-z_]+)\s*\(", text)))


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built: run `make -C game-of-life-distributed_amd/csrc` "
                                "or __graft_entry__.build()")
    lib = ctypes.CDLL(path)
    H = ctypes.c_void_p
    i32, i64, u32, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
    P = ctypes.POINTER
    sig = {
        "golhip_version": ([], ctypes.c_char_p),
        "golhip_build_info": ([], ctypes.c_char_p),
        "golhip_last_error": ([], ctypes.c_char_p),
        "golhip_device_count": ([P(i32)], ctypes.c_int),
        "golhip_host_alloc": ([u64, P(ctypes.c_void_p)], ctypes.c_int),
        "golhip_host_free": ([ctypes.c_void_p], ctypes.c_int),
        "golhip_host_link_probe": ([i32, u64, i32, P(ctypes.c_double), P(ctypes.c_double)], ctypes.c_int),
        "golhip_create": ([i32, i32, i32, u32, P(H)], ctypes.c_int),
        "golhip_create_strip": ([i32, i32, i32, i32, i32, u32, P(H)], ctypes.c_int),
        "golhip_destroy": ([H], ctypes.c_int),
        "golhip_set_stream": ([H, ctypes.c_void_p], ctypes.c_int),
        "golhip_stream": ([H], ctypes.c_void_p),
        "golhip_set_tb_depth": ([H, i32], ctypes.c_int),
        "golhip_set_rows_per_wave": ([H, i32], ctypes.c_int),
        "golhip_set_option": ([H, ctypes.c_char_p, i64], ctypes.c_int),
        "golhip_set_pad_step": ([H, i32], ctypes.c_int),
        "golhip_group_set_pad_step": ([P(H), i32, i32], ctypes.c_int),
        "golhip_rule_parse": ([ctypes.c_char_p, P(u32), P(u32)], ctypes.c_int),
        "golhip_rule_format": ([u32, u32, ctypes.c_char_p, u64], ctypes.c_int),
        "golhip_set_rule": ([H, u32, u32], ctypes.c_int),
        "golhip_rule": ([H, P(u32), P(u32)], ctypes.c_int),
        "golhip_set_rule_flips": ([H, i32], ctypes.c_int),
        "golhip_rule_flips": ([H, P(i32)], ctypes.c_int),
        "golhip_set_topology": ([H, i32], ctypes.c_int),
        "golhip_topology": ([H, P(i32)], ctypes.c_int),
        "golhip_rule_parse_ex": ([ctypes.c_char_p, P(u32), P(u32), P(i32), P(i32), P(i32)], ctypes.c_int),
        "golhip_rule_format_ex": ([u32, u32, i32, i32, i32, ctypes.c_char_p, u64], ctypes.c_int),
        "golhip_pattern_rule": ([ctypes.c_char_p, P(u32), P(u32)], ctypes.c_int),
        "golhip_comm_unique_id": ([ctypes.c_char_p], ctypes.c_int),
        "golhip_comm_init": ([H, ctypes.c_char_p, i32, i32], ctypes.c_int),
        "golhip_comm_info": ([H, P(i32), P(i32), P(i32)], ctypes.c_int),
        "golhip_test_ring_init": ([H, i32, i32, i32, TRANSPORT_FN, ctypes.c_void_p], ctypes.c_int),
        "golhip_group_step": ([P(H), i32, i64], ctypes.c_int),
        "golhip_group_step_ex": ([P(H), i32, i64, i32], ctypes.c_int),
        "golhip_halo_plan": ([i32, i32, i32, i32, i32, P(HaloPlan)], ctypes.c_int),
        "golhip_halo_schedule": ([i32, i32, i32, i64, P(i32), P(i32)], ctypes.c_int),
        "golhip_load_bytes": ([H, ctypes.c_void_p], ctypes.c_int),
        "golhip_load_bits": ([H, ctypes.c_void_p], ctypes.c_int),
        "golhip_fill_random": ([H, u64], ctypes.c_int),
        "golhip_step": ([H, i64, i32], ctypes.c_int),
        "golhip_sync": ([H], ctypes.c_int),
        "golhip_turn": ([H, P(i64)], ctypes.c_int),
        "golhip_alive_count": ([H, P(u64), P(i64)], ctypes.c_int),
        "golhip_alive_count_global": ([H, P(u64), P(i64)], ctypes.c_int),
        "golhip_flips": ([H, ctypes.c_void_p, u64, P(u64)], ctypes.c_int),
        "golhip_step_flips": ([H, i64, ctypes.c_void_p, u64, ctypes.c_void_p, P(u64)], ctypes.c_int),
        "golhip_alive_cells": ([H, ctypes.c_void_p, u64, P(u64)], ctypes.c_int),
        "golhip_flip_stream": ([H, i64, i32, ctypes.c_void_p, u64, ctypes.c_void_p, P(i64), P(u64)], ctypes.c_int),
        "golhip_group_flip_stream": ([P(H), i32, i64, i32, ctypes.c_void_p, u64, ctypes.c_void_p, P(i64), P(u64)],
                                     ctypes.c_int),
        "golhip_snapshot_bytes": ([H, ctypes.c_void_p], ctypes.c_int),
        "golhip_snapshot_bits": ([H, ctypes.c_void_p], ctypes.c_int),
        "golhip_snapshot_rows": ([H, i32, i32, ctypes.c_void_p], ctypes.c_int),
        "golhip_board_hash": ([H, P(u64)], ctypes.c_int),
        "golhip_view_frame": ([H, P(View), ctypes.c_void_p, u64, P(i64)], ctypes.c_int),
        "golhip_view_stream": ([H, i64, i64, P(View), ctypes.c_void_p, u64, P(u64), P(i64)], ctypes.c_int),
        "golhip_group_view_frame": ([P(H), i32, P(View), ctypes.c_void_p, u64, P(i64)], ctypes.c_int),
        "golhip_group_view_stream": ([P(H), i32, i64, i64, P(View), ctypes.c_void_p, u64, P(u64), P(i64)],
                                     ctypes.c_int),
        "golhip_checkpoint_begin": ([P(H), i32, ctypes.c_char_p, P(CkptOpts), P(ctypes.c_void_p)], ctypes.c_int),
        "golhip_checkpoint_wait": ([ctypes.c_void_p, P(CkptInfo)], ctypes.c_int),
        "golhip_checkpoint_info": ([ctypes.c_char_p, P(CkptInfo)], ctypes.c_int),
        "golhip_checkpoint_load": ([P(H), i32, ctypes.c_char_p, P(CkptOpts), P(CkptInfo)], ctypes.c_int),
        "golhip_image_begin": ([P(H), i32, ctypes.c_char_p, P(CkptOpts), P(ctypes.c_void_p)], ctypes.c_int),
        "golhip_image_wait": ([ctypes.c_void_p, P(ImageInfo)], ctypes.c_int),
        "golhip_image_info": ([ctypes.c_char_p, P(ImageInfo)], ctypes.c_int),
        "golhip_image_load": ([P(H), i32, ctypes.c_char_p, P(CkptOpts), P(ImageInfo)], ctypes.c_int),
        "golhip_drain_wait": ([P(H), i32], ctypes.c_int),
        "golhip_test_image_expand": ([i32, ctypes.c_void_p, i32, i32, i32, i32, ctypes.c_void_p, u64], ctypes.c_int),
        "golhip_clear": ([H], ctypes.c_int),
        "golhip_stamp_bits": ([H, ctypes.c_void_p, i32, i32, i32, i32, i32], ctypes.c_int),
        "golhip_group_stamp_bits": ([P(H), i32, ctypes.c_void_p, i32, i32, i32, i32, i32], ctypes.c_int),
        "golhip_pattern_info": ([ctypes.c_char_p, P(PatternInfo)], ctypes.c_int),
        "golhip_pattern_read": ([ctypes.c_char_p, ctypes.c_void_p, u64, P(PatternInfo)], ctypes.c_int),
        "golhip_stamp_file": ([P(H), i32, ctypes.c_char_p, i32, i32, i32, P(PatternInfo)], ctypes.c_int),
        "golhip_extract_bits": ([H, i32, i32, i32, i32, ctypes.c_void_p, u64], ctypes.c_int),
        "golhip_group_extract_bits": ([P(H), i32, i32, i32, i32, i32, ctypes.c_void_p, u64], ctypes.c_int),
        "golhip_alive_box": ([P(H), i32, P(i32), P(i32), P(i32), P(i32)], ctypes.c_int),
        "golhip_box_interval": ([ctypes.c_void_p, i32, P(i32), P(i32)], ctypes.c_int),
        "golhip_pattern_write": ([ctypes.c_char_p, ctypes.c_void_p, i32, i32, u32, u32, i32, i32, i64], ctypes.c_int),
        "golhip_save_rle": ([P(H), i32, ctypes.c_char_p, i32, i32, i32, i32, i32, P(PatternInfo)], ctypes.c_int),
        "golhip_perf": ([H, P(Perf)], ctypes.c_int),
        "golhip_perf_reset": ([H], ctypes.c_int),
        "golhip_persist_trace": ([H, P(u64)], ctypes.c_int),
        "golhip_persist_trace_waves": ([H, ctypes.c_void_p, i64], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != GOLHIP_OK:
        raise GolHipError(rc, load().golhip_last_error().decode(errors="replace"))


def device_count() -> int:
    n = ctypes.c_int32(0)
    _check(load().golhip_device_count(ctypes.byref(n)))
    return n.value


CONWAY = (0x008, 0x00C)  # (birth, survive) masks of B3/S23


def rule_parse(text: str) -> tuple[int, int]:
    """golhip_rule_parse: "B36/S23" (either case, either half empty) or the
    legacy "23/36" -> (birth, survive), bit n of each for n alive neighbours."""
    b, s = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _check(load().golhip_rule_parse(text.encode(), ctypes.byref(b), ctypes.byref(s)))
    return b.value, s.value


def rule_format(birth: int, survive: int) -> str:
    """golhip_rule_format: the canonical spelling, digits ascending ("B36/S23")."""
    buf = ctypes.create_string_buffer(32)
    _check(load().golhip_rule_format(birth, survive, buf, len(buf)))
    return buf.value.decode()


TOPOLOGY_TORUS = 0  # GOLHIP_TOPOLOGY_*: the board's edges meet (every new board)
TOPOLOGY_PLANE = 1  # a bounded plane: every cell outside the board is dead for ever


def rule_parse_ex(text: str) -> tuple[int, int, int, int, int]:
    """golhip_rule_parse_ex: rule_parse's spellings with Golly's bounded-grid
    suffix, "B3/S23:P512,512" (plane) or ":T100,7" (torus) -> (birth, survive,
    topology, width, height); without a suffix TOPOLOGY_TORUS and bounds 0."""
    b, s = ctypes.c_uint32(0), ctypes.c_uint32(0)
    t, w, h = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    _check(load().golhip_rule_parse_ex(text.encode(), ctypes.byref(b), ctypes.byref(s), ctypes.byref(t),
                                       ctypes.byref(w), ctypes.byref(h)))
    return b.value, s.value, t.value, w.value, h.value


def rule_format_ex(birth: int, survive: int, topology: int = TOPOLOGY_TORUS, width: int = 0, height: int = 0) -> str:
    """golhip_rule_format_ex: the inverse of rule_parse_ex ("B3/S23:P512,512")."""
    buf = ctypes.create_string_buffer(64)
    _check(load().golhip_rule_format_ex(birth, survive, topology, width, height, buf, len(buf)))
    return buf.value.decode()


def _rule_masks(rule) -> tuple[int, int]:
    return rule_parse(rule) if isinstance(rule, str) else (int(rule[0]), int(rule[1]))


def halo_plan(width: int, strip_rows: int, nranks: int, rank: int, depth: int) -> dict:
    p = HaloPlan()
    _check(load().golhip_halo_plan(width, strip_rows, nranks, rank, depth, ctypes.byref(p)))
    return {k: getattr(p, k) for k, _ in p._fields_}


def halo_schedule(strip_rows: int, tb_depth: int, turns_left: int, resident: bool = False) -> tuple[int, int]:
    """(depth, launches) of the next halo exchange (golhip_halo_schedule)."""
    d, k = ctypes.c_int32(), ctypes.c_int32()
    _check(load().golhip_halo_schedule(strip_rows, tb_depth, 1 if resident else 0, turns_left, ctypes.byref(d),
                                       ctypes.byref(k)))
    return d.value, k.value


class HostArray(np.ndarray):
    """numpy view of golhip_host_alloc memory (page-locked, device-mapped); freed with the array."""

    def __del__(self):
        p = getattr(self, "_golhip_ptr", None)
        if p:
            self._golhip_ptr = None
            try:
                load().golhip_host_free(ctypes.c_void_p(p))
            except Exception:
                pass


def host_array(shape, dtype) -> np.ndarray:
    """A flip buffer the device writes directly (golhip_host_alloc)."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    p = ctypes.c_void_p()
    _check(load().golhip_host_alloc(n, ctypes.byref(p)))
    buf = (ctypes.c_char * n).from_address(p.value)
    a = np.frombuffer(buf, dtype=dt).reshape(shape).view(HostArray)
    a._golhip_ptr = p.value
    return a


def host_link_probe(device: int = 0, nbytes: int = 256 << 20, reps: int = 5) -> dict:
    """The host link into golhip_host_alloc memory (golhip_host_link_probe):
    a kernel's coalesced 16-byte stores (how the event-stream kernel writes
    its entries) and the DMA engine's device-to-host copy, GB/s."""
    k, d = ctypes.c_double(), ctypes.c_double()
    _check(load().golhip_host_link_probe(device, nbytes, reps, ctypes.byref(k), ctypes.byref(d)))
    return {"kernel_write_GBps": round(k.value, 2), "dma_d2h_GBps": round(d.value, 2), "bytes": nbytes, "reps": reps}


def unique_id() -> bytes:
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    _check(load().golhip_comm_unique_id(buf))
    return buf.raw


def _ptr(a: np.ndarray) -> ctypes.c_void_p:
    return ctypes.c_void_p(a.ctypes.data)


class Board:
    """One handle: a whole torus (``rows is None``) or a row strip of it."""

    def __init__(self, width: int, height: int, device: int = 0, *, row0: int = 0, rows: int | None = None,
                 timing: bool = False):
        lib = load()
        self.width, self.height = width, height
        self.row0 = row0
        self.rows = height if rows is None else rows
        self.words = (width + 31) // 32
        h = ctypes.c_void_p()
        flags = FLAG_TIMING if timing else 0
        if rows is None:
            _check(lib.golhip_create(width, height, device, flags, ctypes.byref(h)))
        else:
            _check(lib.golhip_create_strip(width, height, row0, rows, device, flags, ctypes.byref(h)))
        self._h = h

    # lifecycle
    def close(self) -> None:
        if self._h:
            _check(load().golhip_destroy(self._h))
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # configuration
    def set_tb_depth(self, turns: int) -> None:
        _check(load().golhip_set_tb_depth(self._h, turns))

    def set_rows_per_wave(self, rows: int) -> None:
        _check(load().golhip_set_rows_per_wave(self._h, rows))

    def set_option(self, key: str, value: int) -> None:
        _check(load().golhip_set_option(self._h, key.encode(), value))

    def set_pad_step(self, mode: int) -> None:
        """golhip_set_pad_step: widths that are no multiple of 32 on the fast
        kernels as a padded torus: -1 the measured rule (default), 0 never, 1 always."""
        _check(load().golhip_set_pad_step(self._h, mode))

    def set_rule(self, rule) -> None:
        """golhip_set_rule: the Life-like rule of the turns enqueued from now
        on, as "B36/S23" or (birth, survive) masks."""
        b, s = _rule_masks(rule)
        _check(load().golhip_set_rule(self._h, b, s))

    def rule(self) -> tuple[int, int]:
        """golhip_rule: this board's (birth, survive) masks."""
        b, s = ctypes.c_uint32(0), ctypes.c_uint32(0)
        _check(load().golhip_rule(self._h, ctypes.byref(b), ctypes.byref(s)))
        return b.value, s.value

    def set_rule_flips(self, mode: int) -> None:
        """golhip_set_rule_flips: how flip_stream / step_flips run on a board
        with another rule than Conway's: 0 (default) a step and a three-pass
        compaction a turn, 1 the fused turn + list kernel K14.  Same lists."""
        _check(load().golhip_set_rule_flips(self._h, mode))

    def rule_flips(self) -> int:
        """golhip_rule_flips: this board's set_rule_flips mode."""
        m = ctypes.c_int32(0)
        _check(load().golhip_rule_flips(self._h, ctypes.byref(m)))
        return m.value

    def set_topology(self, topology: int) -> None:
        """golhip_set_topology: TOPOLOGY_TORUS (default) or TOPOLOGY_PLANE, the
        bounded plane whose outside is dead for ever, for the turns enqueued
        from now on (any rule, any width, up to 16 turns a launch)."""
        _check(load().golhip_set_topology(self._h, topology))

    def topology(self) -> int:
        """golhip_topology: this board's TOPOLOGY_*."""
        t = ctypes.c_int32(0)
        _check(load().golhip_topology(self._h, ctypes.byref(t)))
        return t.value

    def set_stream(self, stream_ptr: int) -> None:
        _check(load().golhip_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def comm_init(self, uid: bytes, nranks: int, rank: int) -> None:
        _check(load().golhip_comm_init(self._h, uid, nranks, rank))

    def test_ring_init(self, nranks: int, rank: int, ring_rows: int, exchange, allreduce=None) -> None:
        """Test hook (GOLHIP_TEST_HOOKS=1, golhip_test_ring_init): this strip is
        rank `rank` of a ring whose halos move through
        exchange(prev_rank, next_rank, send_up: bytes, send_down: bytes) ->
        (recv_top, recv_bottom) instead of RCCL, and whose
        golhip_alive_count_global sums through allreduce(count: int) -> int
        (the transport call with prev = next = -1)."""
        def cb(_user, prev, nxt, up, down, top, bottom, nbytes):
            try:
                if prev < 0:  # the allreduce of golhip_alive_count_global: one uint64
                    if allreduce is None or nbytes != 8:
                        return 3
                    s = allreduce(int.from_bytes(ctypes.string_at(up, 8), "little")) % (1 << 64)
                    ctypes.memmove(top, s.to_bytes(8, "little"), 8)
                    return 0
                t, b = exchange(prev, nxt, ctypes.string_at(up, nbytes), ctypes.string_at(down, nbytes))
                if len(t) != nbytes or len(b) != nbytes:
                    return 2
                ctypes.memmove(top, t, nbytes)
                ctypes.memmove(bottom, b, nbytes)
                return 0
            except Exception:  # noqa: BLE001 - reported to the library as a failed exchange
                return 1
        self._transport = TRANSPORT_FN(cb)  # kept alive with the handle
        _check(load().golhip_test_ring_init(self._h, nranks, rank, ring_rows, self._transport, None))

    def comm_info(self) -> dict:
        """The ring as RCCL reports it (golhip_comm_info): nranks, rank, ring_rows."""
        n, r, rows = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _check(load().golhip_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(rows)))
        return {"nranks": n.value, "rank": r.value, "ring_rows": rows.value}

    # board I/O
    def load_bytes(self, cells: np.ndarray) -> None:
        c = np.ascontiguousarray(cells, dtype=np.uint8)
        if c.shape != (self.rows, self.width):
            raise ValueError(f"expected {(self.rows, self.width)} bytes, got {c.shape}")
        _check(load().golhip_load_bytes(self._h, _ptr(c)))

    def load_bits(self, words: np.ndarray) -> None:
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if w.shape != (self.rows, self.words):
            raise ValueError(f"expected {(self.rows, self.words)} words, got {w.shape}")
        _check(load().golhip_load_bits(self._h, _ptr(w)))

    def fill_random(self, seed: int) -> None:
        _check(load().golhip_fill_random(self._h, ctypes.c_uint64(seed)))

    # patterns
    def clear(self) -> None:
        """golhip_clear: every cell dead, turn 0."""
        _check(load().golhip_clear(self._h))

    def stamp_bits(self, words, pw: int, ph: int, x0: int, y0: int, op: int = STAMP_COPY) -> None:
        """golhip_stamp_bits: a pw x ph pattern of bit words ((ph, ceil(pw / 32))
        uint32) with its top-left corner at the torus cell (x0, y0).  `words`
        None passes a null pointer (the library refuses it)."""
        if words is None:
            _check(load().golhip_stamp_bits(self._h, None, pw, ph, x0, y0, op))
            return
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if w.size != max(ph, 0) * ((max(pw, 0) + 31) // 32):
            raise ValueError(f"expected {ph} x {(pw + 31) // 32} words, got {w.shape}")
        _check(load().golhip_stamp_bits(self._h, _ptr(w), pw, ph, x0, y0, op))

    def stamp(self, cells, x0: int, y0: int, op: int = STAMP_COPY) -> None:
        """Stamps a 2-D array of cells (alive where a bool is True or a uint8
        is 255) with its top-left corner at the torus cell (x0, y0)."""
        c = _alive_2d(cells)
        self.stamp_bits(pattern_words_np(c), c.shape[1], c.shape[0], x0, y0, op)

    # turn loop
    def step(self, nturns: int, want_flips: bool = False) -> None:
        _check(load().golhip_step(self._h, nturns, 1 if want_flips else 0))

    def stream(self) -> int:
        """The handle's hipStream_t (golhip_stream), e.g. for torch.cuda.ExternalStream."""
        return int(load().golhip_stream(self._h) or 0)

    def sync(self) -> None:
        _check(load().golhip_sync(self._h))

    def turn(self) -> int:
        t = ctypes.c_int64()
        _check(load().golhip_turn(self._h, ctypes.byref(t)))
        return t.value

    # side channels
    def alive_count(self, global_sum: bool = False) -> tuple[int, int]:
        n, t = ctypes.c_uint64(), ctypes.c_int64()
        fn = load().golhip_alive_count_global if global_sum else load().golhip_alive_count
        _check(fn(self._h, ctypes.byref(n), ctypes.byref(t)))
        return n.value, t.value

    def _cells(self, fn) -> np.ndarray:
        n = ctypes.c_uint64()
        rc = fn(self._h, None, 0, ctypes.byref(n))
        if rc not in (GOLHIP_OK, GOLHIP_ERANGE):
            _check(rc)
        xy = np.zeros((max(n.value, 1), 2), dtype=np.int32)
        _check(fn(self._h, _ptr(xy), n.value, ctypes.byref(n)))
        return xy[: n.value]

    def flips(self) -> np.ndarray:
        """(x=col, y=row) pairs, row-major, of cells changed by the last turn."""
        return self._cells(load().golhip_flips)

    def step_flips(self, nturns: int, cap: int, xy: np.ndarray | None = None):
        """Advance nturns turns and return (xy, counts): every turn's flip
        list concatenated in turn order (golhip_step_flips).  Raises
        GolHipError (ERANGE) when the lists exceed cap pairs; the board has
        advanced nturns either way.  A preallocated (>= cap, 2) int32 `xy`
        is filled in place."""
        if xy is None:
            xy = np.empty((max(cap, 1), 2), dtype=np.int32)
        if xy.shape[0] < cap or xy.dtype != np.int32 or not xy.flags.c_contiguous:
            raise ValueError("xy must be a C-contiguous int32 array of >= cap rows")
        counts = np.zeros(max(nturns, 1), dtype=np.uint64)
        n = ctypes.c_uint64()
        _check(load().golhip_step_flips(self._h, nturns, _ptr(xy), cap, _ptr(counts), ctypes.byref(n)))
        return xy[: n.value], counts[:nturns]

    def flip_stream(self, nturns: int, cap: int, fmt: int = FLIPS_XY, out: np.ndarray | None = None):
        """golhip_flip_stream: up to nturns turns with their flip lists, never
        dropping one.  Returns (entries, counts, turns_done): entries are
        (n, 2) int32 (x, y) pairs (FLIPS_XY) or (n,) uint32 cell indices
        y * width + x (FLIPS_INDEX).  Raises GolHipError (ERANGE) when not
        even the first turn fits in cap."""
        shape, dt = ((cap, 2), np.int32) if fmt == FLIPS_XY else ((cap,), np.uint32)
        if out is None:
            out = np.empty((max(cap, 1),) + shape[1:], dtype=dt)
        if out.shape[0] < cap or out.dtype != dt or not out.flags.c_contiguous:
            raise ValueError("out must be a C-contiguous array of >= cap entries")
        counts = np.zeros(max(nturns, 1), dtype=np.uint64)
        done, n = ctypes.c_int64(), ctypes.c_uint64()
        _check(load().golhip_flip_stream(self._h, nturns, fmt, _ptr(out), cap, _ptr(counts), ctypes.byref(done),
                                         ctypes.byref(n)))
        return out[: n.value], counts[: done.value], done.value

    def alive_cells(self) -> np.ndarray:
        return self._cells(load().golhip_alive_cells)

    def snapshot_bytes(self) -> np.ndarray:
        out = np.empty((self.rows, self.width), dtype=np.uint8)
        _check(load().golhip_snapshot_bytes(self._h, _ptr(out)))
        return out

    def snapshot_bits(self) -> np.ndarray:
        out = np.empty((self.rows, self.words), dtype=np.uint32)
        _check(load().golhip_snapshot_bits(self._h, _ptr(out)))
        return out

    def snapshot_rows(self, row: int, nrows: int) -> np.ndarray:
        """Canonical bit words of rows [row, row + nrows) of this handle."""
        out = np.empty((nrows, self.words), dtype=np.uint32)
        _check(load().golhip_snapshot_rows(self._h, row, nrows, _ptr(out)))
        return out

    # saving patterns
    def extract(self, x0: int, y0: int, w: int, h: int) -> np.ndarray:
        """golhip_extract_bits: the w x h cells from the torus cell (x0, y0) on,
        wrapping in x and y, as an (h, w) bool array (a strip: y counts torus
        rows, rows it does not own are False)."""
        return _extract(lambda *a: load().golhip_extract_bits(self._h, *a), x0, y0, w, h)

    def alive_box(self) -> tuple[int, int, int, int]:
        """golhip_alive_box of a whole-torus handle: (x0, y0, w, h), w = h = 0 on an empty board."""
        return group_alive_box([self])

    def board_hash(self) -> int:
        h = ctypes.c_uint64()
        _check(load().golhip_board_hash(self._h, ctypes.byref(h)))
        return h.value

    # live view
    def _view(self, x0, y0, scale, out_w, out_h, fmt) -> View:
        """golhip_view_t; a missing out_w / out_h is the largest that fits."""
        if out_w is None:
            out_w = self.width // max(scale, 1)
        if out_h is None:
            out_h = self.rows // max(scale, 1)
        return View(x0, y0, scale, out_w, out_h, fmt)

    def view_frame(self, x0: int = 0, y0: int = 0, scale: int = 1, out_w: int | None = None,
                   out_h: int | None = None, fmt: int = VIEW_ARGB, out: np.ndarray | None = None):
        """golhip_view_frame: (frame, turn).  The frame is (out_h, out_w) uint32
        (VIEW_ARGB) or uint8 (VIEW_GRAY8), one pixel per scale x scale cells
        from (x0, y0) on; `out` may be a host_array the kernel writes itself."""
        v = self._view(x0, y0, scale, out_w, out_h, fmt)
        dt = np.dtype(np.uint8 if fmt == VIEW_GRAY8 else np.uint32)
        n = max(v.out_w, 0) * max(v.out_h, 0)
        if out is None:
            out = np.empty(max(n, 1), dtype=dt)
        if out.dtype != dt or out.size < n or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {dt} array of >= {n} pixels")
        t = ctypes.c_int64()
        _check(load().golhip_view_frame(self._h, ctypes.byref(v), _ptr(out), out.size * dt.itemsize, ctypes.byref(t)))
        return out.reshape(-1)[:n].reshape(v.out_h, v.out_w), t.value

    def view_stream(self, nturns: int, every: int, x0: int = 0, y0: int = 0, scale: int = 1,
                    out_w: int | None = None, out_h: int | None = None, fmt: int = VIEW_ARGB,
                    out: np.ndarray | None = None, cap_frames: int | None = None):
        """golhip_view_stream: advance nturns turns with a frame behind every
        `every`-th; returns (frames, turns_done), frames (n, out_h, out_w).
        Raises GolHipError (ERANGE, nothing advanced) when `out` (or
        cap_frames) holds fewer than nturns // every frames."""
        v = self._view(x0, y0, scale, out_w, out_h, fmt)
        dt = np.dtype(np.uint8 if fmt == VIEW_GRAY8 else np.uint32)
        n = max(v.out_w, 0) * max(v.out_h, 0)
        if out is None:
            cap = nturns // every if cap_frames is None and every > 0 else (cap_frames or 0)
            out = np.empty(max(cap * n, 1), dtype=dt)
        elif out.dtype != dt or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {dt} array")
        cap = out.size // max(n, 1) if cap_frames is None else min(cap_frames, out.size // max(n, 1))
        nf, done = ctypes.c_uint64(), ctypes.c_int64()
        _check(load().golhip_view_stream(self._h, nturns, every, ctypes.byref(v), _ptr(out), cap, ctypes.byref(nf),
                                         ctypes.byref(done)))
        return out.reshape(-1)[: nf.value * n].reshape(nf.value, v.out_h, v.out_w), done.value

    def perf(self) -> dict:
        p = Perf()
        _check(load().golhip_perf(self._h, ctypes.byref(p)))
        return p.as_dict()

    def persist_trace(self) -> dict:
        """Persistent-kernel diagnostics (set_option("trace", 1) before stepping)."""
        out = (ctypes.c_uint64 * 5)()
        _check(load().golhip_persist_trace(self._h, out))
        band, mx, wait, tot, wgs = (int(x) for x in out)
        return {"band_ticks": band, "max_band_ticks": mx, "wait_ticks": wait, "kernel_ticks": tot, "workgroups": wgs}

    def persist_trace_waves(self, workgroups: int) -> np.ndarray:
        """(start, end) ticks per (workgroup, wave) of one super-step: shape (workgroups, 64, 2)."""
        out = np.zeros(workgroups * 128, dtype=np.uint64)
        _check(load().golhip_persist_trace_waves(self._h, _ptr(out), out.size))
        return out.reshape(workgroups, 64, 2)

    def perf_reset(self) -> None:
        _check(load().golhip_perf_reset(self._h))


def group_step(boards: list[Board], nturns: int, want_flips: bool = False) -> None:
    arr = (ctypes.c_void_p * len(boards))(*[b.handle for b in boards])
    if want_flips:
        _check(load().golhip_group_step_ex(arr, len(boards), nturns, 1))
    else:
        _check(load().golhip_group_step(arr, len(boards), nturns))


def group_set_pad_step(boards: list[Board], mode: int) -> None:
    """golhip_group_set_pad_step: the strips of a group whose width is no
    multiple of 32 on the fast kernels as padded strips: -1 the measured rule
    (default), 0 never, 1 always."""
    arr = (ctypes.c_void_p * len(boards))(*[b.handle for b in boards])
    _check(load().golhip_group_set_pad_step(arr, len(boards), mode))


def group_set_rule(boards: list[Board], rule) -> None:
    """Board.set_rule on every strip of a group (a group's calls need one rule on all)."""
    for b in boards:
        b.set_rule(rule)


def group_set_topology(boards: list[Board], topology: int) -> None:
    """Board.set_topology on every strip of a group (a group's calls need one topology on all)."""
    for b in boards:
        b.set_topology(topology)


def group_set_rule_flips(boards: list[Board], mode: int) -> None:
    """Board.set_rule_flips on every strip of a group (group_flip_stream runs
    fused when every strip has mode 1)."""
    for b in boards:
        b.set_rule_flips(mode)


def group_flip_stream(boards: list[Board], nturns: int, cap: int, fmt: int = FLIPS_XY, out: np.ndarray | None = None):
    """golhip_group_flip_stream: Board.flip_stream of the whole board that the
    strips `boards` (the group of group_step) hold: (entries, counts,
    turns_done), each turn's list row-major over the whole board in global
    coordinates; every strip is left at the same turn.  `out` may be a
    host_array the gather kernels write themselves."""
    shape, dt = ((cap, 2), np.int32) if fmt == FLIPS_XY else ((cap,), np.uint32)
    if out is None:
        out = np.empty((max(cap, 1),) + shape[1:], dtype=dt)
    if out.shape[0] < cap or out.dtype != dt or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous array of >= cap entries")
    counts = np.zeros(max(nturns, 1), dtype=np.uint64)
    done, n = ctypes.c_int64(), ctypes.c_uint64()
    arr = (ctypes.c_void_p * len(boards))(*[b.handle for b in boards])
    _check(load().golhip_group_flip_stream(arr, len(boards), nturns, fmt, _ptr(out), cap, _ptr(counts),
                                           ctypes.byref(done), ctypes.byref(n)))
    return out[: n.value], counts[: done.value], done.value


def _group_view(boards, x0, y0, scale, out_w, out_h, fmt) -> View:
    """golhip_view_t of the strips' whole board; a missing out_w / out_h is the largest that fits."""
    if not boards:
        raise ValueError("no boards")
    if out_w is None:
        out_w = boards[0].width // max(scale, 1)
    if out_h is None:
        out_h = boards[0].height // max(scale, 1)
    return View(x0, y0, scale, out_w, out_h, fmt)


def group_view_frame(boards: list[Board], x0: int = 0, y0: int = 0, scale: int = 1, out_w: int | None = None,
                     out_h: int | None = None, fmt: int = VIEW_ARGB, out: np.ndarray | None = None):
    """golhip_group_view_frame: Board.view_frame of the whole board that the
    strips `boards` (the group of group_step) hold: (frame, turn)."""
    v = _group_view(boards, x0, y0, scale, out_w, out_h, fmt)
    dt = np.dtype(np.uint8 if fmt == VIEW_GRAY8 else np.uint32)
    n = max(v.out_w, 0) * max(v.out_h, 0)
    if out is None:
        out = np.empty(max(n, 1), dtype=dt)
    if out.dtype != dt or out.size < n or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous {dt} array of >= {n} pixels")
    arr = (ctypes.c_void_p * len(boards))(*[b.handle for b in boards])
    t = ctypes.c_int64()
    _check(load().golhip_group_view_frame(arr, len(boards), ctypes.byref(v), _ptr(out), out.size * dt.itemsize,
                                          ctypes.byref(t)))
    return out.reshape(-1)[:n].reshape(v.out_h, v.out_w), t.value


def group_view_stream(boards: list[Board], nturns: int, every: int, x0: int = 0, y0: int = 0, scale: int = 1,
                      out_w: int | None = None, out_h: int | None = None, fmt: int = VIEW_ARGB,
                      out: np.ndarray | None = None, cap_frames: int | None = None):
    """golhip_group_view_stream: Board.view_stream on the strips `boards`:
    (frames, turns_done), frames (n, out_h, out_w)."""
    v = _group_view(boards, x0, y0, scale, out_w, out_h, fmt)
    dt = np.dtype(np.uint8 if fmt == VIEW_GRAY8 else np.uint32)
    n = max(v.out_w, 0) * max(v.out_h, 0)
    if out is None:
        cap = nturns // every if cap_frames is None and every > 0 else (cap_frames or 0)
        out = np.empty(max(cap * n, 1), dtype=dt)
    elif out.dtype != dt or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous {dt} array")
    cap = out.size // max(n, 1) if cap_frames is None else min(cap_frames, out.size // max(n, 1))
    arr = (ctypes.c_void_p * len(boards))(*[b.handle for b in boards])
    nf, done = ctypes.c_uint64(), ctypes.c_int64()
    _check(load().golhip_group_view_stream(arr, len(boards), nturns, every, ctypes.byref(v), _ptr(out), cap,
                                           ctypes.byref(nf), ctypes.byref(done)))
    return out.reshape(-1)[: nf.value * n].reshape(nf.value, v.out_h, v.out_w), done.value


def board_hash_np(words: np.ndarray, row0: int = 0) -> int:
    """Host restatement of golhip_board_hash for parity checks."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    Ww = w.shape[1]
    idx = (np.arange(w.size, dtype=np.uint64) + np.uint64(row0 * Ww))
    x = (idx << np.uint64(32)) | w.reshape(-1).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(z.sum(dtype=np.uint64))


def view_frame_np(words: np.ndarray, width: int, height: int, x0: int = 0, y0: int = 0, scale: int = 1,
                  out_w: int | None = None, out_h: int | None = None, fmt: int = VIEW_ARGB) -> np.ndarray:
    """Host restatement of golhip_view_frame from canonical bit words
    ((height, ceil(width / 32)) uint32): pixel (px, py) counts the alive cells
    n of the scale x scale block from (x0 + px scale, y0 + py scale) on the
    torus and stores g = (255 n + scale^2 - 1) // scale^2 (VIEW_GRAY8, uint8)
    or g * 0x01010101 (VIEW_ARGB, uint32)."""
    s = int(scale)
    if s < 1:
        raise ValueError("scale must be >= 1")
    out_w = width // s if out_w is None else out_w
    out_h = height // s if out_h is None else out_h
    if not (0 <= x0 < width and 0 <= y0 < height and s >= 1 and out_w >= 1 and out_h >= 1
            and out_w * s <= width and out_h * s <= height):
        raise ValueError("view outside one lap of the board")
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(height, -1)
    ys = (y0 + np.arange(out_h * s)) % height
    xs = (x0 + np.arange(out_w * s)) % width
    n = np.zeros((out_h, out_w), dtype=np.int64)
    band = max(1, (1 << 24) // max(out_w * s, 1) // s) * s  # rows unpacked at a time (whole pixel rows)
    for r in range(0, out_h * s, band):
        rows = w[ys[r:r + band]]
        cells = ((rows[:, xs >> 5] >> (xs & 31).astype(np.uint32)) & np.uint32(1)).astype(np.uint8)
        n[r // s:(r + cells.shape[0]) // s] = cells.reshape(-1, s, out_w, s).sum(axis=(1, 3), dtype=np.int64)
    g = (255 * n + s * s - 1) // (s * s)
    if fmt == VIEW_GRAY8:
        return g.astype(np.uint8)
    return (g * 0x01010101).astype(np.uint32)


# --------------------------------------------------------------------------
# the padded torus (golhip_set_pad_step; csrc/gol_pad_plan.h restated in numpy)
# --------------------------------------------------------------------------
def pad_plan_np(width: int) -> tuple[int, int, int]:
    """(Wp, gR, gL) of a width-column board: Wp = roundup(width + 64, 64),
    gR = ceil((Wp - width) / 2) ghost columns behind the last real column,
    gL = Wp - width - gR in front of column 0 (the far end of the wide row)."""
    wp = -(-(width + 64) // 64) * 64
    pad = wp - width
    return wp, (pad + 1) // 2, pad // 2


def pad_src_cols_np(width: int) -> np.ndarray:
    """The real column each of the Wp columns of the wide row holds."""
    wp, gr, _ = pad_plan_np(width)
    c = np.arange(wp, dtype=np.int64)
    return np.where(c < width, c, np.where(c < width + gr, (c - width) % width, (c - wp) % width))


def pad_run_np(board: np.ndarray, turns: int, depth: int, refresh_all: bool = True) -> np.ndarray:
    """The padded torus' schedule on the host: the (H, W) 0/255 board widened
    to Wp columns, then launches of at most `depth` turns of the plain torus
    rule on the Wp x H torus with the ghost columns rewritten from the real
    ones before each (refresh_all False: before the first alone, which goes
    wrong once a stale ghost's error reaches a real column); the real columns
    after `turns` turns."""
    h, w = board.shape
    src = pad_src_cols_np(w)
    wide = (board == 255).astype(np.uint8)[:, src]
    left = turns
    while left > 0:
        d = min(depth, left)
        if refresh_all:
            wide = wide[:, :w][:, src]
        for _ in range(d):
            n = sum(np.roll(np.roll(wide, dr, 0), dc, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1)) - wide
            wide = ((n == 3) | ((wide == 1) & (n == 2))).astype(np.uint8)
        left -= d
    return (wide[:, :w] * 255).astype(np.uint8)


def group_halo_rounds(strip_rows, tb_depth: int, turns: int) -> list[tuple[int, int]]:
    """The (depth, launches) rounds golhip_group_step runs `turns` turns of
    two or more strips of `strip_rows` rows in, at one word per lane:
    golhip_halo_schedule of the group's smallest strip.  (A lone strip is a
    torus with no exchange: the same depths here, one launch a round.)"""
    rounds, left = [], turns
    while left > 0:
        d, k = halo_schedule(min(strip_rows), tb_depth, left)
        if len(strip_rows) == 1:
            k = 1
        rounds.append((d, k))
        left -= d * k
    return rounds


def pad_group_run_np(board: np.ndarray, cuts, turns: int, rounds, seam: str = "window") -> np.ndarray:
    """Padded strips (golhip_group_set_pad_step) on the host: the (H, W) 0/255
    board on the row strips [cuts[i], cuts[i + 1]), each a wide strip of Wp
    columns with HALO_ROWS halo rows above and below.  `rounds` is the (d, k)
    schedule (sum of d k = turns): one exchange of k d wide rows each way, then
    k launches of d turns, launch j over the rows [-e, rows + e) of the strip,
    e = (k - 1 - j) d, from the rows [-(e + d), rows + e + d).  seam: which
    ghosts are rewritten from their row's real columns before a launch --
    "window": every row the launch reads (the scheme); "own": the strip's own
    rows alone (the halo rows keep the neighbour's stale ghosts); "once": the
    window, but before a round's first launch alone.  The real columns after
    `turns` turns."""
    if seam not in ("window", "own", "once"):
        raise ValueError("seam must be window, own or once")
    if sum(d * k for d, k in rounds) != turns:
        raise ValueError("the rounds do not add up to turns")
    h, w = board.shape
    n, hr = len(cuts) - 1, HALO_ROWS
    if n < 1 or cuts[0] != 0 or cuts[-1] != h or any(b <= a for a, b in zip(cuts[:-1], cuts[1:])):
        raise ValueError("cuts must rise from 0 to the board's rows")
    src = pad_src_cols_np(w)
    rows = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    strips = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s = np.zeros((b - a + 2 * hr, len(src)), dtype=np.uint8)
        s[hr:hr + b - a] = (board[a:b] == 255).astype(np.uint8)[:, src]  # the pad pass
        strips.append(s)

    def life(x, wrap_rows):
        p = x if wrap_rows else np.pad(x, ((1, 1), (0, 0)))
        cnt = sum(np.roll(np.roll(p, dr, 0), dc, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1)) - p
        out = ((cnt == 3) | ((p == 1) & (cnt == 2))).astype(np.uint8)
        return out if wrap_rows else out[1:-1]

    def refresh(s, lo, hi):  # rows [lo, hi) relative to the strip's first row
        s[hr + lo:hr + hi] = s[hr + lo:hr + hi, :w][:, src]

    for d, k in rounds:
        x = k * d
        if n > 1:
            if x > hr or x > min(rows):
                raise ValueError("a round exchanges more rows than a strip or its halo holds")
            own = [s[hr:hr + r].copy() for s, r in zip(strips, rows)]
            for i, s in enumerate(strips):
                s[hr - x:hr] = own[(i - 1) % n][-x:]
                s[hr + rows[i]:hr + rows[i] + x] = own[(i + 1) % n][:x]
        for j in range(k):
            e = (k - 1 - j) * d if n > 1 else 0
            for i, s in enumerate(strips):
                lo, hi = (-(e + d), rows[i] + e + d) if n > 1 else (0, rows[i])
                if seam == "window" or (seam == "once" and j == 0):
                    refresh(s, lo, hi)
                elif seam == "own":
                    refresh(s, 0, rows[i])
                win = s[hr + lo:hr + hi].copy()
                for _ in range(d):
                    win = life(win, n == 1)
                if n > 1:  # the rows d inside the window are exact: the launch's outputs
                    s[hr - e:hr + rows[i] + e] = win[d:len(win) - d]
                else:
                    s[hr:hr + rows[i]] = win
    out = np.concatenate([s[hr:hr + r, :w] for s, r in zip(strips, rows)])  # the unpad pass
    return (out * 255).astype(np.uint8)


# --------------------------------------------------------------------------
# checkpoints (golhip_checkpoint_*; the file format is restated in numpy)
# --------------------------------------------------------------------------
CKPT_MAGIC = b"GOLCKPT\x01"
CKPT_HEADER_BYTES = 64


def _handles(boards):
    boards = [boards] if isinstance(boards, Board) else list(boards)
    return (ctypes.c_void_p * len(boards))(*[b.handle for b in boards]), len(boards)


class Checkpoint:
    """A checkpoint in flight (golhip_checkpoint_begin); wait() joins it."""

    def __init__(self, ck):
        self._ck = ck

    def wait(self) -> dict:
        """golhip_checkpoint_wait: the header's fields, file_bytes and the
        timings stall_ms, drain_ms, write_ms.  Raises GolHipError on a file or
        device error (the object is freed either way)."""
        if not self._ck:
            raise ValueError("checkpoint already waited for")
        ck, self._ck = self._ck, None
        info = CkptInfo()
        _check(load().golhip_checkpoint_wait(ck, ctypes.byref(info)))
        return info.as_dict()

    def __del__(self):
        if getattr(self, "_ck", None):
            try:
                load().golhip_checkpoint_wait(self._ck, None)
            except Exception:
                pass
            self._ck = None


def checkpoint_begin(boards, path: str, chunk_rows: int = 0) -> Checkpoint:
    """golhip_checkpoint_begin of one whole-torus Board or the strips of
    group_step: returns at once; the file is complete after .wait()."""
    arr, n = _handles(boards)
    ck = ctypes.c_void_p()
    opts = CkptOpts(chunk_rows)
    _check(load().golhip_checkpoint_begin(arr, n, os.fsencode(path), ctypes.byref(opts), ctypes.byref(ck)))
    return Checkpoint(ck)


def checkpoint_info(path: str) -> dict:
    """golhip_checkpoint_info: header fields and file_bytes (no device needed)."""
    info = CkptInfo()
    _check(load().golhip_checkpoint_info(os.fsencode(path), ctypes.byref(info)))
    d = info.as_dict()
    return {k: d[k] for k in ("width", "height", "turn", "alive", "hash", "file_bytes")}


def checkpoint_load(boards, path: str, chunk_rows: int = 0) -> dict:
    """golhip_checkpoint_load into one Board or a group of strips: board and
    turn come from the file, verified against its count and digest."""
    arr, n = _handles(boards)
    info = CkptInfo()
    opts = CkptOpts(chunk_rows)
    _check(load().golhip_checkpoint_load(arr, n, os.fsencode(path), ctypes.byref(opts), ctypes.byref(info)))
    d = info.as_dict()
    return {k: d[k] for k in ("width", "height", "turn", "alive", "hash", "file_bytes")}


def _splitmix64_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def checkpoint_header_np(width: int, height: int, turn: int, alive: int, digest: int) -> bytes:
    """The 64 header bytes of a checkpoint file (include/golhip.h)."""
    ww = (width + 31) // 32
    q = np.zeros(8, dtype="<u8")
    q[0] = int.from_bytes(CKPT_MAGIC, "little")
    q[1] = 1 | (CKPT_HEADER_BYTES << 32)
    q[2] = width | (height << 32)
    q[3] = turn % (1 << 64)
    q[4] = alive
    q[5] = digest
    q[6] = ww
    with np.errstate(over="ignore"):
        q[7] = _splitmix64_np(q[:7] + np.arange(7, dtype=np.uint64)).sum(dtype=np.uint64)
    return q.tobytes()


def checkpoint_write_np(path: str, words: np.ndarray, width: int, height: int, turn: int) -> None:
    """Writes a checkpoint file from canonical bit words ((height,
    ceil(width / 32)) uint32, padding bits zero) with numpy alone."""
    ww = (width + 31) // 32
    w = np.ascontiguousarray(words, dtype="<u4").reshape(height, ww)
    alive = int(np.unpackbits(w.view(np.uint8)).sum(dtype=np.int64))
    with open(path, "wb") as f:
        f.write(checkpoint_header_np(width, height, turn, alive, board_hash_np(w)))
        f.write(w.tobytes())


def checkpoint_read_np(path: str, verify: bool = True):
    """(info, words) of a checkpoint file, checked as golhip_checkpoint_load
    checks it (ValueError names the failed check; verify=False skips the
    payload's count and digest): info has width, height,
    turn, alive, hash, file_bytes; words are (height, ceil(width / 32)) uint32."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < CKPT_HEADER_BYTES:
        raise ValueError(f"file size: {len(data)} bytes, less than the 64-byte header")
    q = np.frombuffer(data[:CKPT_HEADER_BYTES], dtype="<u8")
    if data[:8] != CKPT_MAGIC:
        raise ValueError("magic: not a GOLCKPT file")
    if int(q[1]) != (1 | (CKPT_HEADER_BYTES << 32)):
        raise ValueError("version")
    with np.errstate(over="ignore"):
        if int(_splitmix64_np(q[:7] + np.arange(7, dtype=np.uint64)).sum(dtype=np.uint64)) != int(q[7]):
            raise ValueError("header check")
    width, height, ww = int(q[2]) & 0xFFFFFFFF, int(q[2]) >> 32, int(q[6])
    if width < 1 or height < 1 or ww != (width + 31) // 32:
        raise ValueError("header check: impossible geometry")
    if len(data) != CKPT_HEADER_BYTES + 4 * height * ww:
        raise ValueError(f"file size: {len(data)} bytes, the header's board needs {CKPT_HEADER_BYTES + 4 * height * ww}")
    words = np.frombuffer(data, dtype="<u4", offset=CKPT_HEADER_BYTES).reshape(height, ww).astype(np.uint32)
    info = {"width": width, "height": height, "turn": int(q[3].astype(np.int64)), "alive": int(q[4]), "hash": int(q[5]),
            "file_bytes": len(data)}
    if verify and int(np.unpackbits(words.view(np.uint8)).sum(dtype=np.int64)) != info["alive"]:
        raise ValueError("alive count")
    if verify and board_hash_np(words) != info["hash"]:
        raise ValueError("digest")
    return info, words


# --------------------------------------------------------------------------
# PGM images, streamed (golhip_image_*; the kernel is restated in numpy)
# --------------------------------------------------------------------------
class Image:
    """An image in flight (golhip_image_begin); wait() joins it."""

    def __init__(self, im):
        self._im = im

    def wait(self) -> dict:
        """golhip_image_wait: width, height, turn, alive, file_bytes,
        header_bytes and the timings stall_ms, drain_ms, write_ms.  Raises
        GolHipError on a file or device error (the object is freed either way)."""
        if not self._im:
            raise ValueError("image already waited for")
        im, self._im = self._im, None
        info = ImageInfo()
        _check(load().golhip_image_wait(im, ctypes.byref(info)))
        return info.as_dict()

    def __del__(self):
        if getattr(self, "_im", None):
            try:
                load().golhip_image_wait(self._im, None)
            except Exception:
                pass
            self._im = None


def image_begin(boards, path: str, chunk_rows: int = 0) -> Image:
    """golhip_image_begin of one whole-torus Board or the strips of group_step:
    returns at once; the PGM file is complete after .wait()."""
    arr, n = _handles(boards)
    im = ctypes.c_void_p()
    opts = CkptOpts(chunk_rows)
    _check(load().golhip_image_begin(arr, n, os.fsencode(path), ctypes.byref(opts), ctypes.byref(im)))
    return Image(im)


def drain_wait(boards) -> None:
    """golhip_drain_wait: the last checkpoint or image begun on these boards
    has left the device (a following begin does not wait inside the call)."""
    arr, n = _handles(boards)
    _check(load().golhip_drain_wait(arr, n))


def image_info(path: str) -> dict:
    """golhip_image_info: width, height, header_bytes and file_bytes of a PGM
    file, checked as the reference's reader checks it (no device needed)."""
    info = ImageInfo()
    _check(load().golhip_image_info(os.fsencode(path), ctypes.byref(info)))
    d = info.as_dict()
    return {k: d[k] for k in ("width", "height", "header_bytes", "file_bytes")}


def image_load(boards, path: str, chunk_rows: int = 0) -> dict:
    """golhip_image_load into one Board or a group of strips, chunk by chunk:
    turn 0, alive <=> byte 255; `alive` is the boards' count after the load."""
    arr, n = _handles(boards)
    info = ImageInfo()
    opts = CkptOpts(chunk_rows)
    _check(load().golhip_image_load(arr, n, os.fsencode(path), ctypes.byref(opts), ctypes.byref(info)))
    d = info.as_dict()
    return {k: d[k] for k in ("width", "height", "alive", "header_bytes", "file_bytes")}


def image_header_np(width: int, height: int) -> bytes:
    """The header of the reference's PGM files (gol/io.go writePgmImage)."""
    return b"P5\n%d %d\n255\n" % (width, height)


def image_expand_np(words: np.ndarray, width: int, row0: int, nrows: int) -> bytes:
    """What the image kernel (K9) writes for the rows [row0, row0 + nrows) of
    canonical bit words ((rows, ceil(width / 32)) uint32): nrows * width
    bytes, row-major, 255 where the cell's bit is set and 0 elsewhere."""
    ww = (width + 31) // 32
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1, ww)[row0:row0 + nrows]
    out = np.zeros((w.shape[0], width), dtype=np.uint8)
    for x in range(width):  # bit x % 32 of word x // 32
        out[:, x] = np.where((w[:, x >> 5] >> np.uint32(x & 31)) & np.uint32(1), 255, 0)
    return out.tobytes()


def image_expand_hook(words: np.ndarray, width: int, row0: int, nrows: int, guard_bytes: int = 64,
                      guard: int = 0xA5, device: int = 0) -> tuple[bytes, bytes]:
    """Test hook (GOLHIP_TEST_HOOKS=1, golhip_test_image_expand): the image
    kernel alone on `words`; returns (its nrows * width bytes, the guard_bytes
    bytes behind them, which the caller filled with `guard`)."""
    ww = (width + 31) // 32
    w = np.ascontiguousarray(words, dtype="<u4").reshape(-1, ww)
    out = np.full(nrows * width + guard_bytes, guard, dtype=np.uint8)
    _check(load().golhip_test_image_expand(device, _ptr(w), width, w.shape[0], row0, nrows, _ptr(out), out.nbytes))
    return out[:nrows * width].tobytes(), out[nrows * width:].tobytes()

# --------------------------------------------------------------------------
# patterns
# --------------------------------------------------------------------------
def _alive_2d(cells) -> np.ndarray:
    """A 2-D bool array: alive where a bool is True or a uint8 is 255."""
    c = np.asarray(cells)
    if c.ndim != 2:
        raise ValueError(f"cells must be a 2-D array, got shape {c.shape}")
    if c.dtype == np.bool_:
        return c
    if c.dtype == np.uint8:
        return c == 255
    raise ValueError(f"cells must be bool or uint8, got {c.dtype}")


def pattern_words_np(cells) -> np.ndarray:
    """The bit words golhip_stamp_bits takes: (ph, ceil(pw / 32)) uint32, cell
    (r, c) = bit c % 32 of word c // 32 of row r, padding bits zero."""
    c = _alive_2d(cells)
    ph, pw = c.shape
    ww = (pw + 31) // 32
    bits = np.zeros((ph, ww * 32), dtype=np.uint8)
    bits[:, :pw] = c
    return np.packbits(bits, axis=1, bitorder="little").view("<u4").astype(np.uint32).reshape(ph, ww)


def group_stamp(boards: list[Board], cells, x0: int, y0: int, op: int = STAMP_COPY) -> None:
    """golhip_group_stamp_bits: Board.stamp on the board held by a group of strips."""
    c = _alive_2d(cells)
    w = pattern_words_np(c)
    arr, n = _handles(boards)
    _check(load().golhip_group_stamp_bits(arr, n, _ptr(w), c.shape[1], c.shape[0], x0, y0, op))


def pattern_info(path: str) -> dict:
    """golhip_pattern_info: width, height, alive and format ("rle" / "pgm") of a pattern file (no device)."""
    info = PatternInfo()
    _check(load().golhip_pattern_info(os.fsencode(path), ctypes.byref(info)))
    return info.as_dict()


def pattern_rule(path: str) -> tuple[int, int]:
    """golhip_pattern_rule: the (birth, survive) masks an RLE file's header
    names; Conway's where it names none or the file is a PGM (no device)."""
    b, s = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _check(load().golhip_pattern_rule(os.fsencode(path), ctypes.byref(b), ctypes.byref(s)))
    return b.value, s.value


def pattern_read(path: str) -> np.ndarray:
    """golhip_pattern_read: the pattern file's cells as a (height, width) bool array (no device)."""
    info = PatternInfo()
    lib = load()
    probe = np.zeros(1, dtype=np.uint32)
    rc = lib.golhip_pattern_read(os.fsencode(path), _ptr(probe), 0, ctypes.byref(info))
    if rc not in (GOLHIP_OK, GOLHIP_ERANGE):
        _check(rc)
    ww = (info.width + 31) // 32
    words = np.zeros((info.height, ww), dtype=np.uint32)
    _check(lib.golhip_pattern_read(os.fsencode(path), _ptr(words), words.size, ctypes.byref(info)))
    bits = np.unpackbits(words.astype("<u4").view(np.uint8).reshape(info.height, ww * 4), axis=1, bitorder="little")
    return bits[:, :info.width].astype(bool)


def stamp_file(boards, path: str, x0: int, y0: int, op: int = STAMP_OR) -> dict:
    """golhip_stamp_file: a pattern file onto one Board or a group of strips; returns pattern_info's dict."""
    arr, n = _handles(boards)
    info = PatternInfo()
    _check(load().golhip_stamp_file(arr, n, os.fsencode(path), x0, y0, op, ctypes.byref(info)))
    return info.as_dict()


# saving patterns
def _words_to_cells(words: np.ndarray, pw: int) -> np.ndarray:
    ph, ww = words.shape
    bits = np.unpackbits(words.astype("<u4").view(np.uint8).reshape(ph, ww * 4), axis=1, bitorder="little")
    return bits[:, :pw].astype(bool)


def _extract(call, x0: int, y0: int, w: int, h: int) -> np.ndarray:
    ww = (max(w, 0) + 31) // 32
    words = np.zeros((max(h, 0), ww), dtype=np.uint32)
    _check(call(x0, y0, w, h, _ptr(words) if words.size else None, words.size))
    return _words_to_cells(words, w)


def group_extract(boards: list[Board], x0: int, y0: int, w: int, h: int) -> np.ndarray:
    """golhip_group_extract_bits: Board.extract on the board held by a group of strips."""
    arr, n = _handles(boards)
    return _extract(lambda *a: load().golhip_group_extract_bits(arr, n, *a), x0, y0, w, h)


def group_alive_box(boards) -> tuple[int, int, int, int]:
    """golhip_alive_box: (x0, y0, w, h) of the smallest box of at most one lap
    around every alive cell of the torus held by one Board or a group of
    strips; w = h = 0 on an empty board."""
    arr, n = _handles(boards)
    v = [ctypes.c_int32(0) for _ in range(4)]
    _check(load().golhip_alive_box(arr, n, *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


def box_interval(bits, n: int | None = None) -> tuple[int, int]:
    """golhip_box_interval: (start, len) of the shortest cyclic interval over
    every True of `bits`, a 1-D bool array of the axis' n positions (no device)."""
    b = np.asarray(bits, dtype=bool).ravel()
    n = b.size if n is None else n
    padded = np.zeros(((max(n, 1) + 31) // 32) * 32, dtype=np.uint8)
    padded[:b.size] = b
    words = np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)
    s, l = ctypes.c_int32(0), ctypes.c_int32(0)
    _check(load().golhip_box_interval(_ptr(words), n, ctypes.byref(s), ctypes.byref(l)))
    return s.value, l.value


def pattern_write(path: str, cells, rule=None, x0: int = 0, y0: int = 0, turn: int = 0) -> None:
    """golhip_pattern_write: a 2-D array of cells as an RLE file whose header
    names `rule` ("B36/S23" or masks; None: Conway's) and whose #CXRLE line
    carries x0, y0 and turn (no device)."""
    c = _alive_2d(cells)
    w = pattern_words_np(c)
    b, s = CONWAY if rule is None else _rule_masks(rule)
    _check(load().golhip_pattern_write(os.fsencode(path), _ptr(w), c.shape[1], c.shape[0], b, s, x0, y0, turn))


def save_rle(boards, path: str, box=None, chunk_rows: int = 0) -> dict:
    """golhip_save_rle: the rectangle box = (x0, y0, w, h) of one Board or a
    group of strips (None: the alive box) as an RLE file, chunk_rows rows at a
    time; returns pattern_info's dict as the writer counted it."""
    arr, n = _handles(boards)
    x0, y0, w, h = (0, 0, 0, 0) if box is None else box
    info = PatternInfo()
    _check(load().golhip_save_rle(arr, n, os.fsencode(path), x0, y0, w, h, chunk_rows, ctypes.byref(info)))
    return info.as_dict()


# Numpy restatements for the tests; they share no code with the C++.
def extract_np(board_cells, x0: int, y0: int, w: int, h: int) -> np.ndarray:
    """What an extract returns: the w x h cells of the (H, W) board from the
    torus cell (x0, y0) on, wrapping in x and y, as a bool array."""
    alive = _alive_2d(np.asarray(board_cells))
    H, W = alive.shape
    return alive[np.ix_((y0 + np.arange(h)) % H, (x0 + np.arange(w)) % W)]


def _interval_np(occ: np.ndarray) -> tuple[int, int]:
    """The shortest cyclic interval over every True, the smallest start among
    equals: a shortest interval starts on a True, so every True is tried as
    the start and the interval must reach the True farthest ahead of it."""
    n = occ.size
    p = np.flatnonzero(occ)
    if p.size == 0:
        return 0, 0
    length = ((p[None, :] - p[:, None]) % n).max(axis=1) + 1
    k = int(np.argmin(length))  # (the first of equals: p ascends)
    return int(p[k]), int(length[k])


def alive_box_np(board_cells) -> tuple[int, int, int, int]:
    """What golhip_alive_box returns for the (H, W) board: (x0, y0, w, h)."""
    alive = _alive_2d(np.asarray(board_cells))
    if not alive.any():
        return 0, 0, 0, 0
    x0, w = _interval_np(alive.any(axis=0))
    y0, h = _interval_np(alive.any(axis=1))
    return x0, y0, w, h


def life_like_np(cells: np.ndarray, birth: int, survive: int, turns: int = 1) -> np.ndarray:
    """`turns` turns of the Life-like rule (birth, survive) on a torus of 0/255
    bytes: bit n of `birth` brings a dead cell with n alive neighbours (of 8)
    to life, bit n of `survive` keeps an alive one."""
    a = (np.asarray(cells) == 255).astype(np.uint8)
    bt = np.array([(birth >> n) & 1 for n in range(9)], dtype=np.uint8)
    st = np.array([(survive >> n) & 1 for n in range(9)], dtype=np.uint8)
    for _ in range(turns):
        rows = a + np.roll(a, 1, axis=0) + np.roll(a, -1, axis=0)
        n = rows + np.roll(rows, 1, axis=1) + np.roll(rows, -1, axis=1) - a
        a = np.where(a == 1, st[n], bt[n]).astype(np.uint8)
    return a * np.uint8(255)


def life_like_plane_np(cells: np.ndarray, birth: int, survive: int, turns: int = 1) -> np.ndarray:
    """life_like_np on a bounded plane: every cell outside the (H, W) board is
    dead at every turn (zero padding, no wrap)."""
    a = (np.asarray(cells) == 255).astype(np.uint8)
    bt = np.array([(birth >> n) & 1 for n in range(9)], dtype=np.uint8)
    st = np.array([(survive >> n) & 1 for n in range(9)], dtype=np.uint8)
    for _ in range(turns):
        p = np.pad(a, 1)
        rows = p[:-2, :] + p[1:-1, :] + p[2:, :]
        n = rows[:, :-2] + rows[:, 1:-1] + rows[:, 2:] - a
        a = np.where(a == 1, st[n], bt[n]).astype(np.uint8)
    return a * np.uint8(255)


def rle_parse_np(text: str) -> np.ndarray:
    """The cells of RLE text as a (y, x) bool array.  Raises ValueError where
    the library refuses the file."""
    lines = text.split("\n")
    k = 0
    while k < len(lines) and (lines[k].strip() == "" or lines[k].lstrip().startswith("#")):
        k += 1
    head = re.fullmatch(r"x=(-?\d+),y=(-?\d+)(?:,rule=(\S+))?", "".join(lines[k].split()) if k < len(lines) else "")
    if not head:
        raise ValueError("no header")
    w, h, rule = int(head.group(1)), int(head.group(2)), head.group(3)
    if rule is not None and re.fullmatch(r"(.*?)(:[TtPp][1-9]\d*,[1-9]\d*)?", rule).group(1).upper() not in ("B3/S23", "23/3"):
        raise ValueError("rule")
    if not (1 <= w < 2 ** 31 and 1 <= h < 2 ** 31):
        raise ValueError("size")
    body = "".join("".join(lines[k + 1:]).split())
    if "!" not in body:
        raise ValueError("no !")
    body = body[:body.index("!")]
    cells = np.zeros((h, w), dtype=bool)
    x = y = 0
    for cnt, tag in re.findall(r"(\d*)(\D)", body):
        n = int(cnt) if cnt else 1
        if tag == "$":
            y, x = y + n, 0
        elif tag in "bo":
            if y >= h or x + n > w:
                raise ValueError("run leaves the box")
            if tag == "o":
                cells[y, x:x + n] = True
            x += n
        else:
            raise ValueError("unknown character")
    return cells


def rle_format_np(cells) -> str:
    """RLE text of a 2-D array of cells: header, runs with trailing dead cells
    and rows left out, lines of at most 70 characters."""
    c = _alive_2d(cells)
    h, w = c.shape
    toks, pending = [], 0  # pending: row ends not yet written
    for y in range(h):
        row = c[y]
        if row.any():
            if pending:
                toks.append(("$", pending))
                pending = 0
            last = int(np.flatnonzero(row)[-1])
            x = 0
            while x <= last:
                e = x
                while e <= last and row[e] == row[x]:
                    e += 1
                toks.append(("o" if row[x] else "b", e - x))
                x = e
        pending += 1
    out, line = [f"x = {w}, y = {h}, rule = B3/S23"], ""
    for tag, n in toks + [("!", 1)]:
        t = (str(n) if n > 1 else "") + tag
        if len(line) + len(t) > 70:
            out.append(line)
            line = ""
        line += t
    out.append(line)
    return "\n".join(out) + "\n"


def stamp_np(board_cells, cells, x0: int, y0: int, op: int = STAMP_COPY) -> np.ndarray:
    """What a stamp leaves: a copy of the (H, W) board (bool, or uint8 with 255
    alive; the result has the same dtype) with the pattern merged at the
    torus cell (x0, y0), wrapping in x and y."""
    b = np.array(board_cells, copy=True)
    alive = _alive_2d(b).copy()
    p = _alive_2d(cells)
    H, W = alive.shape
    ys = (y0 + np.arange(p.shape[0])) % H
    xs = (x0 + np.arange(p.shape[1])) % W
    cur = alive[np.ix_(ys, xs)]
    new = {STAMP_COPY: p, STAMP_OR: cur | p, STAMP_XOR: cur ^ p, STAMP_CLEAR: cur & ~p}[op]
    alive[np.ix_(ys, xs)] = new
    if b.dtype == np.bool_:
        return alive
    return np.where(alive, 255, 0).astype(np.uint8)


# --------------------------------------------------------------------------
# host mirror of gol.Run (libgolhost.so, include/golrun.h)
# --------------------------------------------------------------------------
HOST_LIB_PATH = os.environ.get("GOLHOST_LIB") or os.path.join(HERE, "libgolhost.so")  # A/B builds
FLAG_KEYS, FLAG_REF_QUIRKS, FLAG_NO_CELL_EVENTS, FLAG_NO_TURN_EVENTS, FLAG_VIEW_STRIPS = 0x1, 0x2, 0x4, 0x8, 0x10
FLAG_SAVE_RLE = 0x20  # GOLRUN_FLAG_SAVE_RLE
FLAG_RULE_FLIPS = 0x40  # GOLRUN_FLAG_RULE_FLIPS
FLAG_PLANE = 0x80  # GOLRUN_FLAG_PLANE
ALIVE_CELLS_COUNT, IMAGE_OUTPUT_COMPLETE, STATE_CHANGE, CELL_FLIPPED, TURN_COMPLETE, FINAL_TURN_COMPLETE = range(6)
PAUSED, EXECUTING, QUITTING = range(3)
EVENT_NAMES = ["AliveCellsCount", "ImageOutputComplete", "StateChange", "CellFlipped", "TurnComplete",
               "FinalTurnComplete"]


class RunEvent(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32), ("new_state", ctypes.c_int32), ("completed_turns", ctypes.c_int64),
        ("cells_count", ctypes.c_int64), ("cell_x", ctypes.c_int64), ("cell_y", ctypes.c_int64),
        ("alive_len", ctypes.c_int64), ("filename", ctypes.c_char * 256), ("text", ctypes.c_char * 288),
    ]


class RunOpts(ctypes.Structure):
    """golrun_opts_t"""
    _fields_ = [("view", ctypes.POINTER(View)), ("view_every", ctypes.c_int32), ("reserved0", ctypes.c_int32),
                ("checkpoint_path", ctypes.c_char_p), ("checkpoint_every", ctypes.c_int64),
                ("resume_path", ctypes.c_char_p), ("reserved", ctypes.c_int64 * 4)]


class DrainStats(ctypes.Structure):
    _fields_ = [("count", ctypes.c_uint64 * 6), ("last_turn", ctypes.c_int64), ("final_alive", ctypes.c_int64)]


_host = None


def load_host(path: str = HOST_LIB_PATH) -> ctypes.CDLL:
    global _host
    if _host is not None:
        return _host
    load()
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built")
    lib = ctypes.CDLL(path)
    P = ctypes.POINTER
    i32, i64, u32, u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
    sig = {
        "golrun_last_error": ([], ctypes.c_char_p),
        "golrun_start": ([i64, i64, i64, i64, ctypes.c_char_p, i32, u32, i32, i32, P(ctypes.c_void_p)], ctypes.c_int),
        "golrun_start_view": ([i64, i64, i64, i64, ctypes.c_char_p, i32, u32, i32, i32, P(View), i32,
                               P(ctypes.c_void_p)], ctypes.c_int),
        "golrun_start_opts": ([i64, i64, i64, i64, ctypes.c_char_p, i32, u32, i32, i32, P(RunOpts),
                               P(ctypes.c_void_p)], ctypes.c_int),
        "golrun_view_frame": ([ctypes.c_void_p, ctypes.c_void_p, u64, P(i64)], ctypes.c_int),
        "golrun_event_string": ([P(RunEvent), ctypes.c_char_p, u64], ctypes.c_int),
        "golrun_next_event": ([ctypes.c_void_p, P(RunEvent), i32], ctypes.c_int),
        "golrun_event_cells": ([ctypes.c_void_p, ctypes.c_void_p, u64], ctypes.c_int),
        "golrun_send_key": ([ctypes.c_void_p, u32], ctypes.c_int),
        "golrun_drain": ([ctypes.c_void_p, P(DrainStats), ctypes.c_void_p, ctypes.c_void_p, i64, i64], ctypes.c_int),
        "golrun_wait": ([ctypes.c_void_p, ctypes.c_char_p, u64], ctypes.c_int),
        "golrun_destroy": ([ctypes.c_void_p], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _host = lib
    return lib


class Run:
    """`go gol.Run(p, events, keyPresses)`; iterate it like `for event := range events`.

    Events are dicts: {"type": "TurnComplete", "CompletedTurns": 3, ...}."""

    def __init__(self, turns: int, threads: int, width: int, height: int, root: str, *, device: int = 0,
                 keys: bool = False, quirks: bool = False, cell_events: bool = True, turn_events: bool = True,
                 events_cap: int = 0, ticker_ms: int = 0, view: dict | None = None, checkpoint: dict | None = None,
                 resume: str | None = None, stream_images: bool = False, image_every: int = 0, blank: bool = False,
                 patterns=None, rule=None, save_rle: bool = False, rule_flips: bool = False, plane: bool = False):
        """view: the live view (golrun_start_view), dict(scale=..., every=1,
        x0=0, y0=0, out_w=None, out_h=None, fmt=VIEW_ARGB, strips=False);
        missing out_w / out_h are the largest that fit.  Run.view_frame()
        fetches frames.  strips=True lets a run on row strips (GOL_STRIPS /
        GOL_NGPU) render its view across them; without it such a run is refused.
        checkpoint: dict(path=..., every=0): a checkpoint file at every turn
        that is a multiple of `every`, and on `q` one of the turn the run stops
        at.  resume: a checkpoint file the run starts from, at its turn
        (golrun_start_opts).  stream_images: images/ and out/ files through
        golhip_image_* (the load in chunks, every image written behind the
        turns); image_every: with it, out/<W>x<H>x<turn>.pgm at every turn that
        is a multiple of it.  blank: start from an empty board instead of
        images/<W>x<H>.pgm.  patterns: [(path, x, y[, op]), ...], pattern
        files (RLE or PGM) stamped in order, top-left corner at the torus cell
        (x, y), after the initial board is there and before any event; op is
        "copy", "or" (the default), "xor" or "clear" (or a STAMP_* number).
        rule: the run's Life-like rule, "B36/S23" or (birth, survive) masks
        (None: Conway's); a resumed run names it again, pattern files must
        name it or none.  save_rle: beside the final image and the images of
        `s` and `q`, out/<W>x<H>x<turn>.rle with the alive box of the board
        (golhip_save_rle), complete before that image's ImageOutputComplete; an
        empty board writes none.  rule_flips: the CellFlipped events of a run
        with another rule than Conway's come from the fused turn + list kernel
        (golhip_set_rule_flips 1 on every handle); the events are the same.
        plane: the board is a bounded plane, every cell outside it dead for ever
        (golhip_set_topology on every handle and strip); same kinds of events."""
        lib = load_host()
        rule_word = 0
        if rule is not None:
            rb, rs = _rule_masks(rule)
            if not (0 <= rb <= 0x1FF and 0 <= rs <= 0x1FF):
                raise ValueError("rule masks above 0x1FF")
            rule_word = 0 if (rb, rs) == CONWAY else 0x40000 | rs << 9 | rb
        flags = (FLAG_KEYS if keys else 0) | (FLAG_REF_QUIRKS if quirks else 0) | \
            (0 if cell_events else FLAG_NO_CELL_EVENTS) | (0 if turn_events else FLAG_NO_TURN_EVENTS) | \
            (FLAG_SAVE_RLE if save_rle else 0) | (FLAG_RULE_FLIPS if rule_flips else 0) | \
            (FLAG_PLANE if plane else 0)
        more = checkpoint is not None or resume is not None or stream_images or image_every != 0 or blank or \
            bool(patterns) or rule_word != 0  # golrun_start_opts
        spec = None
        if patterns:
            ops = {STAMP_COPY: "copy", STAMP_OR: "or", STAMP_XOR: "xor", STAMP_CLEAR: "clear"}
            rows = []
            for pat in patterns:
                if len(pat) not in (3, 4) or "\n" in os.fspath(pat[0]):
                    raise ValueError("a pattern is (path, x, y[, op])")
                op = pat[3] if len(pat) == 4 else "or"
                rows.append(f"{os.fspath(pat[0])}@{int(pat[1])},{int(pat[2])},{ops.get(op, op)}")
            spec = ctypes.create_string_buffer("\n".join(rows).encode())
        h = ctypes.c_void_p()
        self._view = None
        if checkpoint is not None and (set(checkpoint) - {"path", "every"} or "path" not in checkpoint):
            raise ValueError("checkpoint needs path (and every)")
        if view is None and not more:
            rc = lib.golrun_start(turns, threads, width, height, root.encode(), device, flags, events_cap, ticker_ms,
                                  ctypes.byref(h))
        else:
            ro = RunOpts()
            ro.view_every = 1
            if checkpoint is not None:
                ro.checkpoint_path = os.fsencode(checkpoint["path"])
                ro.checkpoint_every = int(checkpoint.get("every", 0))
            if resume is not None:
                ro.resume_path = os.fsencode(resume)
            ro.reserved[0] = int(image_every)
            ro.reserved[1] = 1 if stream_images else 0
            ro.reserved[2] = ctypes.addressof(spec) if spec is not None else 0  # (copied before the call returns)
            ro.reserved[3] = 1 if blank else 0
            ro.reserved0 = rule_word
        if view is not None:
            unknown = set(view) - {"scale", "every", "x0", "y0", "out_w", "out_h", "fmt", "strips"}
            if unknown or "scale" not in view:
                raise ValueError(f"view needs scale; unknown keys {sorted(unknown)}")
            s = int(view["scale"])
            ow, oh = view.get("out_w"), view.get("out_h")
            self._view = View(view.get("x0", 0), view.get("y0", 0), s, width // max(s, 1) if ow is None else ow,
                              height // max(s, 1) if oh is None else oh, view.get("fmt", VIEW_ARGB))
            if view.get("strips"):
                flags |= FLAG_VIEW_STRIPS
            if not more:
                rc = lib.golrun_start_view(turns, threads, width, height, root.encode(), device, flags, events_cap,
                                           ticker_ms, ctypes.byref(self._view), int(view.get("every", 1)),
                                           ctypes.byref(h))
            else:
                ro.view = ctypes.pointer(self._view)
                ro.view_every = int(view.get("every", 1))
        if more:
            rc = lib.golrun_start_opts(turns, threads, width, height, root.encode(), device, flags, events_cap,
                                       ticker_ms, ctypes.byref(ro), ctypes.byref(h))
        if rc != 0:
            raise GolHipError(rc, lib.golrun_last_error().decode())
        self._h = h
        self._ev = RunEvent()

    def next(self, timeout_ms: int = -1):
        """Next event dict, None once closed, "timeout" on timeout."""
        lib = load_host()
        rc = lib.golrun_next_event(self._h, ctypes.byref(self._ev), timeout_ms)
        if rc == 0:
            return None
        if rc == 2:
            return "timeout"
        if rc != 1:
            raise GolHipError(rc, lib.golrun_last_error().decode())
        e = self._ev
        ev = {"type": EVENT_NAMES[e.kind], "CompletedTurns": e.completed_turns, "String": e.text.decode()}
        if e.kind == ALIVE_CELLS_COUNT:
            ev["CellsCount"] = e.cells_count
        elif e.kind == IMAGE_OUTPUT_COMPLETE:
            ev["Filename"] = e.filename.decode()
        elif e.kind == STATE_CHANGE:
            ev["NewState"] = e.new_state
        elif e.kind == CELL_FLIPPED:
            ev["Cell"] = (e.cell_x, e.cell_y)
        elif e.kind == FINAL_TURN_COMPLETE:
            xy = np.zeros((max(e.alive_len, 1), 2), dtype=np.int64)
            rc = lib.golrun_event_cells(self._h, _ptr(xy), e.alive_len)
            if rc != 0:
                raise GolHipError(rc, lib.golrun_last_error().decode())
            ev["Alive"] = xy[: e.alive_len]
        return ev

    def __iter__(self):
        while True:
            ev = self.next()
            if ev is None:
                return
            yield ev

    def drain(self, turns_cap: int = 0, width: int = 0):
        """main.go's headless drain loop in C++ (golrun_drain): consume every
        event until close.  Returns (counts by event name, last TurnComplete,
        len(FinalTurnComplete.Alive), per-turn CellFlipped counts, per-turn
        ordered digests)."""
        st = DrainStats()
        flips = np.zeros(max(turns_cap, 1), dtype=np.uint64)
        dig = np.zeros(max(turns_cap, 1), dtype=np.uint64)
        rc = load_host().golrun_drain(self._h, ctypes.byref(st), _ptr(flips) if turns_cap else None,
                                      _ptr(dig) if turns_cap else None, turns_cap, width)
        if rc != 0:
            raise GolHipError(rc, load_host().golrun_last_error().decode())
        counts = {EVENT_NAMES[k]: int(st.count[k]) for k in range(6)}
        return counts, st.last_turn, st.final_alive, flips[:turns_cap], dig[:turns_cap]

    def view_frame(self):
        """golrun_view_frame: (frame, turn), a copy of the newest published
        frame ((out_h, out_w) uint32 or uint8) and the turn its pixels show."""
        v = self._view
        if v is None:
            raise ValueError("the run was started without a view")
        out = np.empty((v.out_h, v.out_w), dtype=np.uint8 if v.format == VIEW_GRAY8 else np.uint32)
        t = ctypes.c_int64(-1)
        rc = load_host().golrun_view_frame(self._h, _ptr(out), out.nbytes, ctypes.byref(t))
        if rc != 0:
            raise GolHipError(rc, load_host().golrun_last_error().decode())
        return out, t.value

    def send_key(self, key: str) -> None:
        lib = load_host()
        rc = lib.golrun_send_key(self._h, ord(key))
        if rc != 0:
            raise GolHipError(rc, lib.golrun_last_error().decode())

    def wait(self) -> str:
        """Join the run; returns the panic message ('' if the run ended normally)."""
        buf = ctypes.create_string_buffer(1024)
        load_host().golrun_wait(self._h, buf, 1024)
        return buf.value.decode()

    def close(self) -> None:
        if self._h:
            load_host().golrun_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
