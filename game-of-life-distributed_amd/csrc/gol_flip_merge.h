// gol_flip_merge.h — golhip_group_flip_stream's merge plan: where every
// strip's per-turn flip segment goes in the board's list.  Host arithmetic
// only (no HIP), so tests/test_group_flips_cpu.py compiles it on its own.
#pragma once
#include <cstdint>
#include <vector>

namespace gh __attribute__((visibility("hidden"))) {

struct FlipMergePlan {
    int64_t done = 0;              // turns delivered: the first `done` turns fit in cap
    uint64_t total = 0;            // entries of those turns
    uint64_t need = 0;             // entries of turn `done` (the one that did not fit; 0 when all did)
    uint64_t most = 0;             // the largest board count among the delivered turns
    uint64_t max_seg = 0;          // the longest single (turn, strip) segment among them
    std::vector<uint64_t> counts;  // [done]: the board's count of turn t
    std::vector<uint64_t> goff;    // [n][T] (strip-major): strip i's turn-t segment starts at entry goff[i * T + t]
};

// runs[i * (T + 1) + t]: entries of strip i's list before turn t (runs[i][0]
// = 0), as K5 leaves them.  A strip that overflowed cap by itself at turn s
// ran no later turn and its bounds past s + 1 are void (zero); the board's
// total passes cap at turn s at the latest, so the scan below stops before it
// reads them (and treats a falling bound as a stop).
// Strip order within a turn is the board's row-major order:
//   goff[t][i] = sum of all strips' counts of the turns < t + sum of the strips' j < i counts of turn t.
inline FlipMergePlan flip_merge_plan(const unsigned long long *runs, int n, int64_t T, uint64_t cap) {
    FlipMergePlan p;
    p.goff.assign((size_t)n * (size_t)T, 0);
    uint64_t acc = 0;
    for (int64_t t = 0; t < T; ++t) {
        uint64_t c = 0;
        bool ok = true;
        for (int i = 0; i < n; ++i) {
            const unsigned long long r0 = runs[(size_t)i * (size_t)(T + 1) + (size_t)t], r1 = runs[(size_t)i * (size_t)(T + 1) + (size_t)t + 1];
            if (r1 < r0) {
                ok = false;
                break;
            }
            c += r1 - r0;
        }
        if (!ok) break;
        if (c > cap || acc > cap - c) {
            p.need = c;
            break;
        }
        uint64_t at = acc;
        for (int i = 0; i < n; ++i) {
            const uint64_t k = runs[(size_t)i * (size_t)(T + 1) + (size_t)t + 1] - runs[(size_t)i * (size_t)(T + 1) + (size_t)t];
            p.goff[(size_t)i * (size_t)T + (size_t)t] = at;
            at += k;
            if (k > p.max_seg) p.max_seg = k;
        }
        p.counts.push_back(c);
        if (c > p.most) p.most = c;
        acc += c;
        p.done = t + 1;
    }
    p.total = acc;
    return p;
}

}  // namespace gh
