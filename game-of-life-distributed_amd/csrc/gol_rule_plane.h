// gol_rule_plane.h — launcher of K15 (gol_rule_plane.hip), K11 on a bounded
// plane: every cell outside [0, W) x [0, H) is dead at every turn of a launch.
// Internal, as gol_rule.h.
#pragma once
#include "gol_rule.h"

namespace golk {

// One launch of `depth` turns (1, 2, 4, 6, 8, 12 or 16, at ANY width: a plane
// has no row seam) of the rule (birth, survive), as launch_step_rule; brow0 is
// the board row of the frame's output row 0 (a strip's row0 plus the launch's
// first row, negative for a deep-halo launch of the first strip) and H the
// board's rows.  Rows outside [0, H) are read through a.in like any other
// (the addresses stay valid) and count as dead.
hipError_t launch_step_plane(const StepArgs &a, int depth, uint32_t birth, uint32_t survive, int brow0, int H,
                             hipStream_t s, bool dyn = false);
// Resident waves per CU of the instance launch_step_plane would take.
int plane_wave_slots_per_cu(int depth, uint32_t birth, uint32_t survive, bool dyn);

}  // namespace golk
