// Issue-rate probe: the pair rule's patterns in loops of 5-37 KB,
// with the waves of a CU pair started at different times (desync), timed by the
// kernel's events and by the older wave's own loop.
//   hipcc -O3 --offload-arch=gfx950 -o desync_probe scripts/desync_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

#define CLOB "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63"
#define B3(d, a, b, c) "v_bitop3_b32 v" #d ", v" #a ", v" #b ", v" #c " bitop3:0x96\n"
#define DPP(d, a) "v_mov_b32_dpp v" #d ", v" #a " wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
#define ALB(d, a, b) "v_alignbit_b32 v" #d ", v" #a ", v" #b ", 31\n"


#define P_s3_unit B3(40,48,49,50) B3(41,49,50,51) B3(42,50,51,52) DPP(44,60) B3(43,51,52,53) B3(40,52,53,54) B3(41,53,54,55) ALB(45,61,44) B3(42,45,55,56) B3(43,55,56,57) B3(40,56,57,58) DPP(46,62) B3(41,57,58,59) B3(42,58,59,60) B3(43,59,60,61) ALB(47,63,46) B3(40,47,49,50) B3(41,49,50,51) B3(42,50,51,52) DPP(44,60) B3(43,51,52,53) B3(40,52,53,54) B3(41,53,54,55) ALB(45,61,44) B3(42,45,55,56) B3(43,55,56,57) B3(40,56,57,58) B3(41,57,58,59) B3(42,58,59,60) B3(43,59,60,61) B3(40,48,49,50) DPP(46,62) B3(41,49,50,51) B3(42,50,51,52) B3(43,51,52,53) ALB(47,63,46) B3(40,47,53,54) B3(41,53,54,55) B3(42,54,55,56) B3(43,55,56,57)
#define P_gap3_5 B3(40,48,49,50) B3(41,49,50,51) B3(42,50,51,52) DPP(44,60) B3(43,51,52,53) B3(40,52,53,54) B3(41,53,54,55) ALB(45,61,44) B3(42,45,55,56) B3(43,55,56,57) B3(40,56,57,58) DPP(46,62) B3(41,57,58,59) B3(42,58,59,60) B3(43,59,60,61) ALB(47,63,46) B3(40,47,49,50) B3(41,49,50,51) B3(42,50,51,52) B3(43,51,52,53) B3(40,52,53,54) DPP(44,60) B3(41,53,54,55) B3(42,54,55,56) B3(43,55,56,57) B3(40,56,57,58) B3(41,57,58,59) ALB(45,61,44) B3(42,45,59,60) B3(43,59,60,61) B3(40,48,49,50) B3(41,49,50,51) B3(42,50,51,52) DPP(46,62) B3(43,51,52,53) B3(40,52,53,54) B3(41,53,54,55) B3(42,54,55,56) B3(43,55,56,57) ALB(47,63,46)
#define P_grouped DPP(44,60) DPP(46,62) ALB(45,61,44) B3(40,45,49,50) ALB(47,63,46) B3(41,47,50,51) B3(42,50,51,52) B3(43,51,52,53) B3(40,52,53,54) B3(41,53,54,55) B3(42,54,55,56) B3(43,55,56,57) B3(40,56,57,58) B3(41,57,58,59) B3(42,58,59,60) B3(43,59,60,61) DPP(44,60) DPP(46,62) ALB(45,61,44) ALB(47,63,46) B3(40,47,49,50) B3(41,49,50,51) B3(42,50,51,52) B3(43,51,52,53) B3(40,52,53,54) B3(41,53,54,55) B3(42,54,55,56) B3(43,55,56,57) B3(40,56,57,58) B3(41,57,58,59) B3(42,58,59,60) B3(43,59,60,61) B3(40,48,49,50) B3(41,49,50,51) B3(42,50,51,52) B3(43,51,52,53) B3(40,52,53,54) B3(41,53,54,55) B3(42,54,55,56) B3(43,55,56,57)
constexpr int nlines(const char* t) { int n = 0; for (; *t; ++t) n += *t == '\n'; return n; }
// block at 4 (mod 32); REPT copies of the 40-instruction pattern in the loop; desync: wave w of
// (block parity, wave) starts w x ~0.8 us late, so the waves of a CU pair sit at different code addresses
#define KERNEL(name, rept, body)                                                   \
    constexpr int name##_n = nlines(body) * rept;                                        \
    __global__ void name(int iters, long long* sink, int desync) {                           \
        const int w = (threadIdx.x >> 6) + 8 * (blockIdx.x & 1);                    \
        if (desync) for (int i = 0; i < w * desync; ++i) __builtin_amdgcn_s_sleep(30);        \
        const long long c0 = clock64(), w0 = wall_clock64();                      \
        for (int i = 0; i < iters; ++i) asm volatile(".p2align 5\ns_nop 0\n.rept " #rept "\n" body ".endr\n" ::: CLOB); \
        const long long c1 = clock64(), w1 = wall_clock64();                      \
        if (threadIdx.x == 0) { sink[2 * blockIdx.x] = c1 - c0; sink[2 * blockIdx.x + 1] = w1 - w0; } \
    }
KERNEL(k_win_16, 16, P_s3_unit)
KERNEL(k_win_58, 58, P_s3_unit)
KERNEL(k_win_116, 116, P_s3_unit)
KERNEL(k_grp_16, 16, P_grouped)
KERNEL(k_grp_58, 58, P_grouped)
KERNEL(k_grp_116, 116, P_grouped)
KERNEL(k_g35_58, 58, P_gap3_5)
typedef void (*kfn)(int, long long*, int);
int main(int argc, char** argv) {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    long long* sink;
    CK(hipMalloc(&sink, 16 * cus));
    long long* hs = (long long*)malloc(16 * cus);
    struct { const char* n; kfn f; int len; int rept; } ks[] = {{"window x16", k_win_16, k_win_16_n, 16}, {"window x58", k_win_58, k_win_58_n, 58},
        {"window x116", k_win_116, k_win_116_n, 116}, {"grouped x16", k_grp_16, k_grp_16_n, 16}, {"grouped x58", k_grp_58, k_grp_58_n, 58},
        {"grouped x116", k_grp_116, k_grp_116_n, 116}, {"gap3_5 x58", k_g35_58, k_g35_58_n, 58}};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int rep = 0; rep < 2; ++rep)
    for (int desync : {0, 1})
        for (auto& k : ks) {
            const int wps = 2, threads = 64 * 4 * wps, iters = 64000 / k.rept;
            hipLaunchKernelGGL(k.f, dim3(cus), dim3(threads), 0, 0, 10, sink, desync);
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(k.f, dim3(cus), dim3(threads), 0, 0, iters, sink, desync);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            CK(hipMemcpy(hs, sink, 16 * cus, hipMemcpyDeviceToHost));
            // in-kernel: cycles and 100 MHz ticks of wave 0's loop alone (the start delays are outside it)
            double cyc = 0, wall = 0;
            for (int b = 0; b < cus; ++b) cyc += hs[2 * b], wall += hs[2 * b + 1];
            const double inst = double(iters) * k.len;           // instructions of one wave
            const double us = wall / cus / 100.0;                // its loop time
            printf("%-13s desync %d  wave0 loop %.1f us  kernel %.1f us  clock %.3f GHz  winst/SIMD-cycle (2.4 GHz): by wave 0's loop %.4f, by the kernel %.4f\n",
                   k.n, desync, us, ms * 1e3, cyc / wall * 0.1, 2 * inst / (us * 1e-6) / 2.4e9, 2 * inst / (ms * 1e-3) / 2.4e9);
        }
    return 0;
}
