// lqr_wave1.hip -- gfx950 launch of lqr_wave1_body.h: a 16-lane row per problem, the problem in LDS, for n_ctrl = 1,
// n_state <= 6, float32 (pendulum / cart-pole iLQR at the batch sizes it is run at: the lane-per-problem kernel then
// has a handful of wavefronts on the whole chip and its time is one lane's instruction count).
#include "lqr_common.h"
#include "lqr_wave1_wv.h"
#include "lqr_wave1_body.h"

namespace mpclqr {
namespace {

template <int NS>
__global__ void __launch_bounds__(64) lqr_step_wave1_kernel(StepParams<float> p)
{
    wave1::step_wave<NS>(p);
}

template <int NS> int launch_ns(const StepParams<float> &p, hipStream_t st)
{
    const size_t lds = (size_t)wave1::layout(p).total * 16;      // four problems
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&lqr_step_wave1_kernel<NS>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((lqr_step_wave1_kernel<NS>), dim3((unsigned)((p.B + 3) / 4)), dim3(64), lds, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error(hipGetErrorString(e));
        return MPC_E_LAUNCH;
    }
    return MPC_OK;
}

}  // namespace

bool wave1_supported(const StepParams<float> &p) { return wave1::shape_supported(p); }
long wave1_lds_bytes(const StepParams<float> &p) { return (long)wave1::layout(p).total * 16; }

int launch_step_wave1(const StepParams<float> &p, hipStream_t st)
{
    switch (p.ns) {
    case 1: return launch_ns<1>(p, st);
    case 2: return launch_ns<2>(p, st);
    case 3: return launch_ns<3>(p, st);
    case 4: return launch_ns<4>(p, st);
    case 5: return launch_ns<5>(p, st);
    case 6: return launch_ns<6>(p, st);
    }
    set_last_error("wave-per-problem kernel: n_state out of range");
    return MPC_E_DIMS;
}

}  // namespace mpclqr
