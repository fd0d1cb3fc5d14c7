// lqr_wave1_carry.hip -- the CARRY instantiation of lqr_wave1_body.h (-DMPC_WAVE1_CARRY, impl 10): a 16-lane row per problem for a
// shipped simulator behind MPC_ENV_CTRL_CARRY -- the slew-rate augmentation z = (u_prev, x), n_state = 4 (pendulum, both variants) or
// 6 (cart-pole), n_ctrl = 1, float32.  The lane-per-problem kernel (impl 4), the only other one that carries the control, has B / 64
// wavefronts on the chip; this one has B / 4.  Forced only: impl 0 never picks it, impl 6 (lqr_wave1.hip) refuses the flag as ever.
#ifndef MPC_WAVE1_CARRY
#error "lqr_wave1_carry.hip is compiled with -DMPC_WAVE1_CARRY (csrc/Makefile)"
#endif
#include "lqr_common.h"
#include "lqr_wave1_wv.h"
#include "lqr_wave1_body.h"

namespace mpclqr {
namespace {

template <int NS>
__global__ void __launch_bounds__(64) lqr_step_wave1_carry_kernel(StepParams<float> p)
{
    wave1::step_wave<NS>(p);
}

template <int NS> int launch_ns(const StepParams<float> &p, hipStream_t st)
{
    const size_t lds = (size_t)wave1::layout(p).total * 16;      // four problems
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&lqr_step_wave1_carry_kernel<NS>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((lqr_step_wave1_carry_kernel<NS>), dim3((unsigned)((p.B + 3) / 4)), dim3(64), lds, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error(hipGetErrorString(e));
        return MPC_E_LAUNCH;
    }
    return MPC_OK;
}

}  // namespace

bool wave1_carry_supported(const StepParams<float> &p) { return wave1::shape_supported(p); }
long wave1_carry_lds_bytes(const StepParams<float> &p) { return (long)wave1::layout(p).total * 16; }

int launch_step_wave1_carry(const StepParams<float> &p, hipStream_t st)
{
    if (!wave1::shape_supported(p)) {                   // (the route asked already: nothing reaches the kernels that they do not take)
        set_last_error("row-per-problem carry kernel: not an augmented simulator step");
        return MPC_E_DIMS;
    }
    switch (p.ns) {
    case 4: return launch_ns<4>(p, st);
    case 6: return launch_ns<6>(p, st);
    }
    set_last_error("row-per-problem carry kernel: n_state out of range");
    return MPC_E_DIMS;
}

}  // namespace mpclqr
