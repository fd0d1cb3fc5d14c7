// lqr_wave1_wv.h -- the `wv::` lane interface of lqr_wave1_body.h for gfx950: a 64-lane wavefront of four 16-lane rows, the LDS as an
// array of floats, DPP row broadcasts.  Shared by lqr_wave1.hip and lqr_wave1_carry.hip (tests/emu/ implements the same names with
// lockstep fibers).
#pragma once
#include "lqr_common.h"
// lane, problem, bcast, ballot, any, ctz64 are the shared ones; lds_sync and fmac_bcast are bound below for this kernel (wv_gfx950.h says
// under "the names a kernel binds for itself" how they differ), so the header's asm forms of them are left out
#define MPC_WV_ROW_PER_PROBLEM
#include "wv_gfx950.h"

namespace mpclqr {
namespace wv {
extern __shared__ float g_sm[];
MPC_DEV float &sm(int i) { return g_sm[i]; }
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
// the workgroup is this one wavefront and its LDS instructions execute in order: the phases only have to be kept apart
MPC_DEV void lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
}  // namespace wv
}  // namespace mpclqr
