// gol_plane_mask.h — the two masks that make K15 (gol_rule_plane.hip) a
// bounded plane: which bits of a tile lane's word are columns of the board,
// and whether a row of a launch's frame is a row of the board.  Everything
// outside [0, W) x [0, H) is dead at every turn of a launch.
//
// Plain C++ on purpose (no HIP header): the host tests compile this file with
// g++ and check it exhaustively (tests/test_plane_cpu.py); the kernel calls the
// same functions.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GOL_PLANE_HD __host__ __device__ __forceinline__
#else
#define GOL_PLANE_HD inline
#endif

namespace golk {

// The columns of the board in word `wi` of a row of W cells (Ww = ceil(W / 32)
// words): every bit of a word wholly inside, the low W % 32 bits of the row's
// last word where W % 32 != 0, none for a word index outside [0, Ww) (the
// lanes of a tile that hang over either side of the board).
GOL_PLANE_HD uint32_t plane_col_mask(int wi, int W, int Ww) {
    if (wi < 0 || wi >= Ww) return 0u;
    const int tb = W & 31;
    return (wi == Ww - 1 && tb != 0) ? (1u << tb) - 1u : ~0u;
}

// The word such a lane loads: its own where it has one, else the nearest word
// of the row (never wrapped, never out of bounds; its mask is 0).
GOL_PLANE_HD int plane_col_clamp(int wi, int Ww) { return wi < 0 ? 0 : wi >= Ww ? Ww - 1 : wi; }

// Whether board row `brow` exists on a board of H rows.
GOL_PLANE_HD bool plane_row_inside(int brow, int H) { return (unsigned)brow < (unsigned)H; }

// The board row of the word leaving stage t (turn t + 1 of the launch) with
// the row that entered the pipeline as board row `brow_in`: each stage emits
// the row before the one entering it.
GOL_PLANE_HD int plane_stage_row(int brow_in, int t) { return brow_in - (t + 1); }

}  // namespace golk
