// gol_rule_flip.h — launcher of K14 (gol_rule_flip.hip): K5's per-launch turn
// + CellFlipped list kernel for any Life-like rule (gol_rule_bits.h).
// Internal, as gol_kernels.h.
#pragma once
#include "gol_kernels.h"

namespace golk {

// K14's kernel argument: K5's, unchanged (FlipTurnArgs keeps its layout, so
// Conway's kernels keep their instruction streams), and the rule's two masks.
struct RuleFlipTurnArgs {
    FlipTurnArgs turn;
    uint32_t birth, survive;
};

// One launch of K14: launch_flip_turn with the rule (birth, survive).  Every
// field of `a` means what it means to K5, the copy blocks included.
// dyn: the dynamic policy even where (birth, survive) has a static instance.
hipError_t launch_rule_flip_turn(const FlipTurnArgs &a, uint32_t birth, uint32_t survive, bool dyn, hipStream_t s);
// Blocks of K14 a CU holds, for the instance launch_rule_flip_turn would take
// (contig: Ww % 4 == 0; odd: W % 32 != 0); 0 if the query fails.
int rule_flip_turn_blocks_per_cu(bool contig, bool odd, uint32_t birth, uint32_t survive, bool dyn);

}  // namespace golk
