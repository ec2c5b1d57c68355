// gol_rule.h — launcher of K11 (gol_rule.hip), the step kernel that takes a
// Life-like rule (gol_rule_bits.h).  Internal, as gol_kernels.h.
#pragma once
#include "gol_kernels.h"

namespace golk {

// Most turns a K11 launch fuses: up to 9 VGPRs of state a stage; at 16 the
// kernels take 106 (static policy) and 115 VGPRs (dynamic) and four waves
// share a SIMD, at 32 two would.
constexpr int kRuleMaxDepth = 16;
// The depths with an instance, 16, 12, 8, 6, 4, 2 and 1, are every depth
// depth_plan returns under that cap (tests/test_gpu_rules.py walks them).

// One launch of `depth` turns of the rule (birth, survive): output rows
// [0, a.rows_out) from input rows [-depth, rows_out + depth) through a.in,
// stored at a.dst_base; a.alive (nullable) += popcount of the output rows in
// [count_lo, count_hi).  Canonical words, one word per lane.  W % 32 == 0:
// one of those depths; any other width: depth 1 (the kernel closes the row
// seam and keeps the bits of columns >= W zero).  a.rows_per_wave >= 1.
// dyn: the dynamic policy even where (birth, survive) has a static instance.
hipError_t launch_step_rule(const StepArgs &a, int depth, uint32_t birth, uint32_t survive, hipStream_t s,
                            bool dyn = false);
// Resident waves per CU of the instance launch_step_rule would take.
int rule_wave_slots_per_cu(int depth, int W, uint32_t birth, uint32_t survive, bool dyn);

}  // namespace golk
