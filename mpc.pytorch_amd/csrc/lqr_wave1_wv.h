// lqr_wave1_wv.h -- the `wv::` lane interface of lqr_wave1_body.h for gfx950: a 64-lane wavefront of four 16-lane rows, the LDS as an
// array of floats, DPP row broadcasts.  Shared by lqr_wave1.hip and lqr_wave1_carry.hip (tests/emu/ implements the same names with
// lockstep fibers).
#pragma once
#include "lqr_common.h"

#define MPC_DEV __device__ __forceinline__

namespace mpclqr {
namespace wv {
extern __shared__ float g_sm[];
MPC_DEV float &sm(int i) { return g_sm[i]; }
MPC_DEV int lane() { return (int)threadIdx.x; }
MPC_DEV int problem() { return (int)blockIdx.x; }
// lane N of the caller's 16-lane row (DPP row_newbcast)
template <int N> MPC_DEV float bcast(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x150 + N, 0xf, 0xf, true));
}
// acc += bcast_N(src) * mul.  A v_mov_b32_dpp and a v_fmac the compiler schedules among the neighbouring chains and
// whose DPP wait states it places itself: measured 4 % faster here than `s_nop 1; v_fmac_f32_dpp` in an asm block it cannot
// see into (57.8 against 60.5 us per cart-pole step).
template <int N> MPC_DEV void fmac_bcast(float &acc, float src, float mul) { acc = fmaf(bcast<N>(src), mul, acc); }
// sum over the sixteen lanes of the row, the same value in all of them
MPC_DEV double row_sum_f64(double x)
{
    for (int off = 8; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
MPC_DEV double shfl_xor_f64(double x, int off) { return __shfl_xor(x, off); }
MPC_DEV double readlane_f64(double x, int src) { return __shfl(x, src); }
MPC_DEV float readlane(float x, int src) { return __shfl(x, src); }
MPC_DEV unsigned long long ballot(bool c) { return __ballot(c); }
MPC_DEV bool any(bool c) { return __ballot(c) != 0ull; }
MPC_DEV int ctz64(unsigned long long m) { return __builtin_ctzll(m); }
// the workgroup is this one wavefront and its LDS instructions execute in order: the phases only have to be kept apart
MPC_DEV void lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
}  // namespace wv
}  // namespace mpclqr
