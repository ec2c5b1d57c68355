// gol_flip_turn.h — the body of K5, one turn fused with its CellFlipped list,
// with the rule as a functor: gol_kernels.hip instantiates it on Conway's
// 3-LUT rule (K5, K5r), gol_rule_flip.hip on the Life-like policies of
// gol_rule_bits.h (K14).  Device code; included by those two files only.
//
// Per block of 256 threads, 1024 consecutive canonical words (word
// k * 256 + tid of the block: every load and board store is a coalesced
// 256-word access):
//   1. the turn: three input rows per word, the column neighbours from the
//      adjacent lanes (DPP; a row's first / last word and the wave's edge
//      lanes load theirs), then the rule functor on the three rows' words
//      with their west / east neighbours aligned;
//   2. flips = old ^ new, counted per word into a packed 4 x 16-bit vector
//      (one field per k) so ONE block scan orders the block's words;
//   3. decoupled look-back (blocks take virtual ids from a ticket, so every
//      predecessor is already running): the block publishes its aggregate,
//      wave 0 reads up to 64 predecessors per step (one lane each) until the
//      nearest one holding an inclusive prefix, then publishes its own;
//      status words are 64-bit agent-scope atomics carrying (flag, epoch,
//      value) together, so there is no separate payload to hand off;
//   4. entries (row-major: word order, then bit order) go to LDS at their
//      block-relative positions and leave in one coalesced copy (blocks
//      with more entries than LDS holds store them directly).
// HBM traffic per turn: the board read once (neighbour words hit L1/L2),
// written once, plus the entries.
#pragma once
#include <type_traits>

#include "gol_kernels.h"
#include "gol_bits.h"
#include "gol_flip_seam.h"

namespace golk {

__device__ __forceinline__ int map_in_row(const RowMap &m, int i) {
    int r = i + m.off;
    if (m.wrap > 0) {
        r %= m.wrap;
        if (r < 0) r += m.wrap;
    }
    return m.base + min(r, m.rmax);
}

constexpr int kFtThreads = 256, kFtK = 4, kFtWords = kFtThreads * kFtK;
// 32 KiB of entry staging: four blocks per CU, so a 5120^2 turn (800 blocks)
// is resident at once; a block with more entries stores them directly.
constexpr int kFtLdsBytes = 32768;
constexpr unsigned long long kFtAgg = 1ull << 62, kFtPrefix = 2ull << 62;
constexpr unsigned long long kFtValMask = (1ull << 40) - 1;

__device__ __forceinline__ unsigned long long ft_word(unsigned long long flag, unsigned epoch, unsigned long long v) {
    return flag | ((unsigned long long)(epoch & 0x3FFFFFu) << 40) | (v & kFtValMask);
}

// nw 32-bit words, device list `src` -> host list `d` (any 4-byte alignment
// of either), by thread gt of gn (>= 3): 16-byte stores to the destination's
// 16-byte boundaries from 4-byte loads, 4-byte heads and tails.
__device__ __forceinline__ void ft_copy_words(uint32_t *d, const uint32_t *src, unsigned long long nw,
                                              unsigned long long gt, unsigned long long gn) {
    const unsigned long long head = min(nw, (unsigned long long)((4u - (unsigned)(((uintptr_t)d >> 2) & 3u)) & 3u));
    const unsigned long long nq = (nw - head) / 4;
    if (gt < head) d[gt] = src[gt];
    for (unsigned long long q = gt; q < nq; q += gn) {
        const unsigned long long w = head + 4 * q;
        *reinterpret_cast<uint4 *>(d + w) = make_uint4(src[w], src[w + 1], src[w + 2], src[w + 3]);
    }
    const unsigned long long t0 = head + 4 * nq;
    if (t0 + gt < nw) d[t0 + gt] = src[t0 + gt];
}

// The copy blocks of a K5 launch: the previous turn's entries, device list
// -> host list, in 16-byte stores to the destination's 16-byte boundaries
// (4-byte heads and tails), spread over the copy blocks.  They never wait on
// anything, so the turn's own blocks keep their co-residency, and their host
// stores are in their own waves: the turn's loads never wait behind them
// (vmcnt is per wave).  Whether the previous turn is delivered follows from
// its run bounds alone (a stop flag set by this launch's own blocks must not
// cancel the copy of a turn that did fit).
__device__ void flip_copy_prev(const FlipTurnArgs &a, unsigned cb, unsigned ncb) {
    const unsigned long long s = a.cp_run[0], e0 = a.cp_run[1];
    if (a.stop_on_overflow && e0 > a.cap) return;  // that turn did not fit: the host rolls back to it
    const unsigned long long e = e0 < a.cap ? e0 : a.cap;
    if (e <= s) return;
    const unsigned wpe = a.format == kFlipFormatXY ? 2u : 1u;  // 32-bit words per entry
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.out) + s * wpe;
    uint32_t *d = reinterpret_cast<uint32_t *>(a.cp_dst) + s * wpe;
    ft_copy_words(d, src, (e - s) * wpe, (unsigned long long)cb * kFtThreads + threadIdx.x,
                  (unsigned long long)ncb * kFtThreads);
}

// Shared memory of one K5 block.
struct FtShared {
    unsigned long long wsum[4], part[4];
    unsigned long long excl;
    int stop;  // K5r: this turn is not delivered (an earlier turn overflowed, or a wait timed out)
    uint32_t alive[4];
    alignas(16) unsigned char buf[kFtLdsBytes];
};

// One block's share of a K5 turn: words vid * 1024 .. + 1023 of the board;
// false when the turn is not delivered (K5r: the block stops).
// CONTIG (Ww % 4 == 0): thread tid of the block owns the 4 consecutive words
// base + 4 tid .. + 3 of one row (16-byte loads and stores); otherwise word
// base + k * 256 + tid for k = 0..3 (4-byte accesses, any Ww).
// SC1 (K5r): every board and entry access is a write-through (sc1) buffer
// access, the hand-off form that needs no fence (MI355X_MICROARCH.md, valid
// forms); the block reports its turn done once its stores have drained.
// ODD (W % 32 != 0): the row seam is closed in the row's first and last word
// (gol_flip_seam.h): a ghost of column 0 in the last word, column W - 1 left
// of the first, and the last word's padding bits cleared after the rule.
// rule(w, x, e): the next word from three rows' words x with their west (w,
// bit b = cell b - 1) and east (e, bit b = cell b + 1) neighbours aligned.  It
// may raise any bit of a lane past the board's end and, ODD, the padding and
// ghost bits of a row's last word (a B0 rule does): both are masked after it.
template <bool CONTIG, bool SC1, bool ODD, class RuleFn>
__device__ __forceinline__ bool flip_turn_block(const FlipTurnArgs &a, const unsigned vid, FtShared &sh,
                                                const RuleFn &rule) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // (unused, and dropped, without SC1)
    const __amdgpu_buffer_rsrc_t srs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(a.src), (short)0, (int)a.board_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(a.dst, (short)0, (int)a.board_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(a.out, (short)0, (int)a.out_bytes, 0x00020000);
    auto src_ld4 = [&](size_t w) -> uint4 {
        if constexpr (SC1) {
            const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(srs, (int)(w * 4), 0, kCpolSc1);
            return make_uint4(v.x, v.y, v.z, v.w);
        } else {
            return *reinterpret_cast<const uint4 *>(a.src + w);
        }
    };
    auto src_ld1 = [&](size_t w) -> uint32_t {
        if constexpr (SC1) return __builtin_amdgcn_raw_buffer_load_b32(srs, (int)(w * 4), 0, kCpolSc1);
        else return a.src[w];
    };
    auto dst_st4 = [&](size_t w, const uint4 &v) {
        if constexpr (SC1) __builtin_amdgcn_raw_buffer_store_b128((v4u32){v.x, v.y, v.z, v.w}, drs, (int)(w * 4), 0, kCpolSc1);
        else *reinterpret_cast<uint4 *>(a.dst + w) = v;
    };
    auto dst_st1 = [&](size_t w, uint32_t v) {
        if constexpr (SC1) __builtin_amdgcn_raw_buffer_store_b32(v, drs, (int)(w * 4), 0, kCpolSc1);
        else a.dst[w] = v;
    };
    auto out_st4 = [&](unsigned long long w, const uint4 &v) {
        if constexpr (SC1) __builtin_amdgcn_raw_buffer_store_b128((v4u32){v.x, v.y, v.z, v.w}, ors, (int)(w * 4), 0, kCpolSc1);
        else *reinterpret_cast<uint4 *>(static_cast<uint32_t *>(a.out) + w) = v;
    };
    auto out_st1 = [&](unsigned long long w, uint32_t v) {
        if constexpr (SC1) __builtin_amdgcn_raw_buffer_store_b32(v, ors, (int)(w * 4), 0, kCpolSc1);
        else static_cast<uint32_t *>(a.out)[w] = v;
    };
    // the turn's run bounds: read by the next turn's blocks and the copy blocks
    // (K5r: stored with kFtRunReady set, which the next turn's blocks wait for)
    auto run_get = [&](int i) {
        return __hip_atomic_load(&a.run[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & ~kFtRunReady;
    };
    auto run_set = [&](unsigned long long v) {
        __hip_atomic_store(&a.run[1], SC1 ? v | kFtRunReady : v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // K5r: this block is done with the turn once every wave's stores have
    // drained (sc1: written through): its own turn count (the next turn's
    // neighbours wait on it), then one count on its shard (the copy blocks)
    auto signal_done = [&]() {
        if constexpr (SC1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                __hip_atomic_store(&a.blk_done[vid], a.turn + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(&a.done[(vid % kFtShards) * kFtShardStride], 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    };
    // K5r: run[0] (this turn's first entry) is the previous turn's last
    // block's prefix: needed only for the entries, so waited for here, not at
    // the turn's start; the last block stores it with kFtRunReady right after
    // its look-back (before its own board and entries).  Thread 0 only.
    auto wait_run = [&]() {
        if constexpr (SC1) {
            if (a.turn > 0) {
                const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
                while (!(__hip_atomic_load(&a.run[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kFtRunReady)) {
                    if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > 200000000ll) {  // 2 s: never
                        atomicOr(&a.ctl[1], 1u);
                        sh.stop = 1;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
        }
    };
    if constexpr (SC1) {
        if (tid == 0) sh.stop = 0;  // (read after the scan's barriers)
    }
    const unsigned Ww = (unsigned)a.Ww;
    const unsigned nwords = (unsigned)a.rows * Ww;  // host: < 2^32
    const unsigned base = vid * (unsigned)kFtWords;
    const unsigned seam_r = (unsigned)a.W & 31u;  // (ODD only: 1..31)

    uint32_t flip[kFtK];
    unsigned long long packed = 0;  // CONTIG: the thread's count in field 0; else one 16-bit field per k
    uint32_t alive_c = 0;
    // K5r holds the new board words until the turn is known to be delivered
    // (no earlier turn of the batch overflowed: that turn's rollback board is
    // the buffer this turn writes)
    uint32_t held[kFtK];
    size_t held_at[kFtK];
    bool held_ok[kFtK];
    if constexpr (CONTIG) {
        const unsigned i0 = base + 4u * (unsigned)tid;
        const bool valid = i0 < nwords;
        const unsigned ii = valid ? i0 : nwords - 4;  // every lane stays active for the DPP moves
        const unsigned y = ii / Ww, c = ii - y * Ww;
        const size_t rows[3] = {(size_t)map_in_row(a.in, (int)y - 1) * Ww, (size_t)map_in_row(a.in, (int)y) * Ww,
                                (size_t)map_in_row(a.in, (int)y + 1) * Ww};
        const unsigned cl = c == 0 ? Ww - 1 : c - 1, cr = c + 4 == Ww ? 0 : c + 4;
        const bool ledge = lane == 0 || c == 0, redge = lane == 63 || c + 4 == Ww;
        // all loads first (the edge words unconditionally: L1 hits beside the 16-B loads)
        uint4 q[3];
        uint32_t le[3], re[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            q[j] = src_ld4(rows[j] + c);
            le[j] = src_ld1(rows[j] + cl);
            re[j] = src_ld1(rows[j] + cr);
        }
        uint32_t x[4][3], wv[4][3], ev[4][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            uint32_t v[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
            if constexpr (ODD) {
                le[j] = c == 0 ? seam_left_word(le[j], seam_r) : le[j];
                v[3] = c + 4 == Ww ? seam_last_word(v[3], re[j], seam_r) : v[3];
            }
            uint32_t l = from_left_lane(v[3]), r = from_right_lane(v[0]);
            l = ledge ? le[j] : l;
            r = redge ? re[j] : r;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                x[k][j] = v[k];
                wv[k][j] = __builtin_amdgcn_alignbit(v[k], k == 0 ? l : v[k - 1], 31);  // bit b = cell b-1
                ev[k][j] = __builtin_amdgcn_alignbit(k == 3 ? r : v[k + 1], v[k], 1);  // bit b = cell b+1
            }
        }
        uint32_t nx[4], cnt = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            nx[k] = rule(wv[k], x[k], ev[k]);
            if constexpr (ODD) {
                if (k == 3) {  // (the ghost bit of x[3][1] goes with the padding)
                    nx[3] = c + 4 == Ww ? seam_clear_pad(nx[3], seam_r) : nx[3];
                    x[3][1] = c + 4 == Ww ? seam_clear_pad(x[3][1], seam_r) : x[3][1];
                }
            }
            flip[k] = valid ? (nx[k] ^ x[k][1]) : 0u;
            cnt += (uint32_t)__builtin_popcount(flip[k]);
            alive_c += valid ? (uint32_t)__builtin_popcount(nx[k]) : 0u;
        }
        if constexpr (SC1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) held[k] = nx[k];
            held_at[0] = (size_t)(a.dst_base + (int)y) * Ww + c;
            held_ok[0] = valid;
        } else {
            if (valid) dst_st4((size_t)(a.dst_base + (int)y) * Ww + c, make_uint4(nx[0], nx[1], nx[2], nx[3]));
        }
        packed = cnt;
    } else {
#pragma unroll
        for (int k = 0; k < kFtK; ++k) {
            const unsigned i = base + (unsigned)(k * kFtThreads + tid);
            const bool valid = i < nwords;
            const unsigned ii = valid ? i : nwords - 1;
            const unsigned y = ii / Ww, c = ii - y * Ww;
            const size_t rows[3] = {(size_t)map_in_row(a.in, (int)y - 1) * Ww, (size_t)map_in_row(a.in, (int)y) * Ww,
                                    (size_t)map_in_row(a.in, (int)y + 1) * Ww};
            const bool ledge = lane == 0 || c == 0, redge = lane == 63 || c == Ww - 1;
            const unsigned cl = c == 0 ? Ww - 1 : c - 1, cr = c == Ww - 1 ? 0 : c + 1;
            uint32_t x[3], le[3], re[3], w[3], e[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                x[j] = src_ld1(rows[j] + c);
                le[j] = src_ld1(rows[j] + cl);
                re[j] = src_ld1(rows[j] + cr);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if constexpr (ODD) {
                    le[j] = c == 0 ? seam_left_word(le[j], seam_r) : le[j];
                    x[j] = c == Ww - 1 ? seam_last_word(x[j], re[j], seam_r) : x[j];
                }
                uint32_t l = from_left_lane(x[j]), r = from_right_lane(x[j]);
                l = ledge ? le[j] : l;
                r = redge ? re[j] : r;
                w[j] = __builtin_amdgcn_alignbit(x[j], l, 31);
                e[j] = __builtin_amdgcn_alignbit(r, x[j], 1);
            }
            uint32_t nx = rule(w, x, e);
            if constexpr (ODD) {  // (the ghost bit of x[1] goes with the padding)
                nx = c == Ww - 1 ? seam_clear_pad(nx, seam_r) : nx;
                x[1] = c == Ww - 1 ? seam_clear_pad(x[1], seam_r) : x[1];
            }
            if constexpr (SC1) {
                held[k] = nx;
                held_at[k] = (size_t)(a.dst_base + (int)y) * Ww + c;
                held_ok[k] = valid;
            } else {
                if (valid) dst_st1((size_t)(a.dst_base + (int)y) * Ww + c, nx);
            }
            flip[k] = valid ? (nx ^ x[1]) : 0u;
            alive_c += valid ? (uint32_t)__builtin_popcount(nx) : 0u;
            packed |= (unsigned long long)__builtin_popcount(flip[k]) << (16 * k);
        }
    }

    // block scan of the packed counts (each field <= 256 x 128 < 2^16)
    unsigned long long inc = packed;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) sh.wsum[wid] = inc;
    if (a.alive) {
        const uint32_t t = wave_sum_u32(alive_c);
        if (lane == 0) sh.alive[wid] = t;
    }
    __syncthreads();
    unsigned long long pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wid) pre += sh.wsum[w];
        tot += sh.wsum[w];
    }
    const unsigned long long excl_packed = pre + inc - packed;
    uint32_t pos[kFtK], T = 0;
    if constexpr (CONTIG) {
        T = (uint32_t)(tot & 0xFFFFu);
        pos[0] = (uint32_t)(excl_packed & 0xFFFFu);
#pragma unroll
        for (int k = 1; k < kFtK; ++k) pos[k] = pos[k - 1] + (uint32_t)__builtin_popcount(flip[k - 1]);
    } else {
#pragma unroll
        for (int k = 0; k < kFtK; ++k) {
            pos[k] = T + (uint32_t)((excl_packed >> (16 * k)) & 0xFFFFu);
            T += (uint32_t)((tot >> (16 * k)) & 0xFFFFu);
        }
    }

    if (a.dbg & 1) {  // measurement only: no look-back (entries overlap)
        if (tid == 0) {
            wait_run();
            const unsigned long long r0 = run_get(0);
            sh.excl = r0;
            if (vid == (unsigned)a.ncompute - 1) run_set(r0);
        }
    } else if (a.coresident) {
        // publish the aggregate, then every thread sums its share of ALL
        // predecessors' aggregates (<= 4 words each at 5120^2): one round of
        // loads instead of a chain of look-back windows
        if (tid == 0)
            __hip_atomic_store(&a.status[vid], ft_word(kFtAgg, a.epoch, T), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long ep = (unsigned long long)(a.epoch & 0x3FFFFFu);
        unsigned long long part = 0;
        for (unsigned j = (unsigned)tid; j < vid; j += kFtThreads) {
            unsigned long long st;
            int spins = 0;
            for (;;) {
                st = __hip_atomic_load(&a.status[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((st >> 62) != 0 && ((st >> 40) & 0x3FFFFFull) == ep) break;
                if (++spins > (1 << 22)) {  // a predecessor never ran: not co-resident after all
                    atomicOr(&a.ctl[1], 1u);
                    st = 0;
                    break;
                }
                if constexpr (SC1) {
                    // K5r: a turn overflowed while this one waits: this is the turn
                    // after it (the blocks that saw the overflow first never start
                    // it, so it never completes): not delivered
                    if ((spins & 63) == 0 && __hip_atomic_load(&a.ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                        sh.stop = 1;
                        st = 0;
                        break;
                    }
                }
                __builtin_amdgcn_s_sleep(1);
            }
            part += st & kFtValMask;
        }
        if ((a.dbg & 4) && tid == 0 && vid == 0) atomicOr(&a.ctl[1], 1u);  // test hook: the fallback
        part = wave_sum_u64(part);
        if (lane == 0) sh.part[wid] = part;
        __syncthreads();
        if (tid == 0) {
            wait_run();
            const unsigned long long excl = run_get(0) + sh.part[0] + sh.part[1] + sh.part[2] + sh.part[3];
            sh.excl = excl;
            if (vid == (unsigned)a.ncompute - 1) {
                const unsigned long long end = excl + T;
                run_set(end);
                if (a.stop_on_overflow && end > a.cap) atomicOr(&a.ctl[0], 1u);
            }
            if (a.alive) {
                const uint32_t al = sh.alive[0] + sh.alive[1] + sh.alive[2] + sh.alive[3];
                if (al) atomicAdd(a.alive, (unsigned long long)al);
            }
        }
    } else if (wid == 0) {
        unsigned long long excl = 0;
        if (vid == 0) {
            excl = run_get(0);
            if (lane == 0)
                __hip_atomic_store(&a.status[0], ft_word(kFtPrefix, a.epoch, excl + T), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0)
                __hip_atomic_store(&a.status[vid], ft_word(kFtAgg, a.epoch, T), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            long long j = (long long)vid - 1 - lane;  // this lane's predecessor
            const unsigned long long ep = (unsigned long long)(a.epoch & 0x3FFFFFu);
            for (;;) {
                unsigned long long st = kFtPrefix;  // lanes past block 0: an empty prefix (never reached)
                if (j >= 0) {
                    int spins = 0;
                    for (;;) {
                        st = __hip_atomic_load(&a.status[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((st >> 62) != 0 && ((st >> 40) & 0x3FFFFFull) == ep) break;
                        if (++spins > (1 << 22)) {  // bounded: record, then treat as an empty prefix
                            atomicOr(&a.ctl[1], 1u);
                            st = kFtPrefix | (ep << 40);
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                }
                const unsigned long long pm = __ballot((st >> 62) == 2);
                if (pm) {
                    const int first = __builtin_ctzll(pm);  // nearest predecessor with an inclusive prefix
                    excl += wave_sum_u64(lane <= first ? (st & kFtValMask) : 0ull);
                    break;
                }
                excl += wave_sum_u64(st & kFtValMask);
                j -= 64;
            }
            if (lane == 0)
                __hip_atomic_store(&a.status[vid], ft_word(kFtPrefix, a.epoch, excl + T), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            sh.excl = excl;
            if (vid == (unsigned)a.ncompute - 1) {  // the last block's inclusive prefix closes the turn
                const unsigned long long end = excl + T;
                run_set(end);
                if (a.stop_on_overflow && end > a.cap) atomicOr(&a.ctl[0], 1u);
            }
            if (a.alive) {
                const uint32_t al = sh.alive[0] + sh.alive[1] + sh.alive[2] + sh.alive[3];
                if (al) atomicAdd(a.alive, (unsigned long long)al);
            }
        }
    }
    __syncthreads();
    if constexpr (SC1) {
        // the turn is delivered unless an earlier turn overflowed (its entries
        // start past cap: the host rolls back to that turn, whose board is the
        // buffer this turn writes) or a wait timed out
        if (tid == 0 && a.stop_on_overflow && run_get(0) > a.cap) sh.stop = 1;
        __syncthreads();
        if (sh.stop) return false;
        if constexpr (CONTIG) {
            if (held_ok[0]) dst_st4(held_at[0], make_uint4(held[0], held[1], held[2], held[3]));
        } else {
#pragma unroll
            for (int k = 0; k < kFtK; ++k)
                if (held_ok[k]) dst_st1(held_at[k], held[k]);
        }
    }
    if (a.dbg & 2) {  // measurement only: no entries
        signal_done();
        return true;
    }
    const unsigned long long bex = sh.excl;
    const int esz = a.format == kFlipFormatXY ? 8 : 4;
    const bool staged = T <= (uint32_t)(kFtLdsBytes / esz);
    auto put = [&](uint32_t p, unsigned x, unsigned y) {
        const unsigned long long gy = (unsigned long long)a.row0 + y;
        if (staged) {
            if (a.format == kFlipFormatXY)
                reinterpret_cast<int2 *>(sh.buf)[p] = make_int2((int)x, (int)gy);
            else
                reinterpret_cast<uint32_t *>(sh.buf)[p] = (uint32_t)(gy * (unsigned)a.W + x);
        } else if (bex + p < a.cap) {
            if (a.format == kFlipFormatXY) {
                out_st1(2 * (bex + p), x);
                out_st1(2 * (bex + p) + 1, (uint32_t)gy);
            } else {
                out_st1(bex + p, (uint32_t)(gy * (unsigned)a.W + x));
            }
        }
    };
#pragma unroll
    for (int k = 0; k < kFtK; ++k) {
        uint32_t m = flip[k];
        if (!m) continue;
        uint32_t p = pos[k];
        const unsigned i = CONTIG ? base + 4u * (unsigned)tid + (unsigned)k : base + (unsigned)(k * kFtThreads + tid);
        const unsigned y = i / Ww, c = i - y * Ww;
        while (m) {
            const int b = __builtin_ctz(m);
            m &= m - 1;
            put(p++, c * 32u + (unsigned)b, y);
        }
    }
    if (!staged) {
        signal_done();
        return true;
    }
    __syncthreads();
    const unsigned long long lim = bex >= a.cap ? 0ull : (a.cap - bex < T ? a.cap - bex : (unsigned long long)T);
    // copy out in 16-byte stores (4 indices or 2 pairs a lane: wider writes
    // when `out` is host memory across PCIe), with 4-byte-word heads and tails
    // up to the 16-byte boundaries of the destination
    const unsigned wpe = (unsigned)esz / 4;                  // 32-bit words per entry
    uint32_t *d = reinterpret_cast<uint32_t *>(a.out) + bex * wpe;
    const uint32_t *sb = reinterpret_cast<const uint32_t *>(sh.buf);
    const unsigned long long nw = lim * wpe;                 // words to copy
    const unsigned long long head = min(nw, (unsigned long long)((4u - (unsigned)(((uintptr_t)d >> 2) & 3u)) & 3u));
    const unsigned long long nq = (nw - head) / 4;           // whole 16-byte groups
    const unsigned long long dw = bex * wpe;                  // d's word offset in `out`
    if ((unsigned long long)tid < head) out_st1(dw + tid, sb[tid]);
    for (unsigned long long q = tid; q < nq; q += kFtThreads) {
        const unsigned long long w = head + 4 * q;
        out_st4(dw + w, make_uint4(sb[w], sb[w + 1], sb[w + 2], sb[w + 3]));
    }
    const unsigned long long t0 = head + 4 * nq;
    if (t0 + (unsigned long long)tid < nw) out_st1(dw + t0 + tid, sb[t0 + tid]);
    signal_done();
    return true;
}

// One block of a per-launch K5 grid (the kernels' whole body).
template <bool CONTIG, bool ODD, class RuleFn>
__device__ __forceinline__ void flip_turn_launch_block(const FlipTurnArgs &a, const RuleFn &rule) {
    // copy blocks first in the grid: dispatched at once, their host stores
    // stream while the turn's blocks compute (behind them, they waited for
    // the whole turn's dispatch: 42 us a 5120^2 turn either way)
    const unsigned ncp = a.cp_run ? (unsigned)a.cp_blocks : 0u;
    if (blockIdx.x < ncp) {
        flip_copy_prev(a, blockIdx.x, ncp);
        return;
    }
    if (a.ctl[0]) return;  // an earlier turn of the batch overflowed: the host rolls back to it
    __shared__ unsigned s_vid;
    __shared__ FtShared sh;
    // Block order: blockIdx when every block is resident at once (no
    // contended counter: 800 returning atomics on one word cost ~9 us);
    // otherwise a ticket, so every predecessor is already running.
    unsigned vid = blockIdx.x - ncp;
    if (!a.coresident) {
        if (threadIdx.x == 0) s_vid = atomicAdd(a.ticket, 1u);
        __syncthreads();
        vid = s_vid;
    }
    flip_turn_block<CONTIG, false, ODD>(a, vid, sh, rule);
}

// Calls f with the (CONTIG, ODD) pair of a board as compile-time constants.
template <class F>
static inline void ft_dispatch(bool contig, bool odd, F &&f) {
    if (contig) {
        if (odd) f(std::true_type{}, std::true_type{});
        else f(std::true_type{}, std::false_type{});
    } else {
        if (odd) f(std::false_type{}, std::true_type{});
        else f(std::false_type{}, std::false_type{});
    }
}

}  // namespace golk
