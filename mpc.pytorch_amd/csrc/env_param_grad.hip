// env_param_grad.hip -- backward of env_linearize_kernel (lqr_generic.hip) with respect to the simulator's parameters:
// per trajectory point the vector-Jacobian product of env_param_grad.h, summed over the N = (T-1) B points.
//
//   env_param_grad_kernel:        one point per lane, grid-stride loop under EPG_MAX_BLOCKS blocks; per-lane sums in double
//                                 (both dtypes), wavefront reduction by cross-lane shuffles, the block's four wavefronts through
//                                 LDS, ONE row of partial sums per block into the workspace.
//   env_param_grad_final_kernel:  one wavefront adds the block rows in a fixed order and writes the np numbers.
//
// No atomics: the grid is a function of N alone and every sum has a fixed order, so the result is bitwise reproducible.
// Every workspace row that is read was written by the first kernel of the same call, the output is written, not
// accumulated into: neither depends on what the buffers held before.
#include <string>

#include "lqr_common.h"
#include "env_param_grad.h"

namespace mpclqr {

namespace {
constexpr int EPG_BLOCK = 256;          // four wavefronts
constexpr int EPG_MAX_BLOCKS = 512;     // two blocks per CU of an MI355X: beyond N = 131072 points the stride loop wraps
constexpr int EPG_ROW = 8;              // doubles per workspace row (np <= 5), 64 bytes

inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error((std::string(what) + ": " + hipGetErrorString(e)).c_str());
        return MPC_E_LAUNCH;
    }
    return MPC_OK;
}
}  // namespace

template <typename real, int KIND>
__global__ __launch_bounds__(EPG_BLOCK) void env_param_grad_kernel(EnvDesc<real> env, long N, const real *__restrict__ x,
                                                                   const real *__restrict__ u, const real *__restrict__ gF,
                                                                   const real *__restrict__ gf, double *__restrict__ ws)
{
    constexpr int ns = EnvKind<KIND>::ns, np = EnvKind<KIND>::np, n = ns + 1;
    real prm[np];
#pragma unroll
    for (int k = 0; k < np; ++k) prm[k] = env.params[k];
    env.params = prm;
    double acc[np];
#pragma unroll
    for (int k = 0; k < np; ++k) acc[k] = 0;
    for (long i = (long)blockIdx.x * EPG_BLOCK + threadIdx.x; i < N; i += (long)gridDim.x * EPG_BLOCK) {
        real xi[ns], gfi[ns], gFi[ns * n], g[np];
#pragma unroll
        for (int j = 0; j < ns; ++j) xi[j] = x[i * ns + j];
#pragma unroll
        for (int j = 0; j < ns; ++j) gfi[j] = gf[i * ns + j];
#pragma unroll
        for (int j = 0; j < ns * n; ++j) gFi[j] = gF[i * (ns * n) + j];
        env_param_vjp<real, KIND>(env, xi, u[i], gFi, gfi, g);
#pragma unroll
        for (int k = 0; k < np; ++k) acc[k] += (double)g[k];
    }
    // lanes of a wavefront (every lane arrives here: the loop has no early exit)
#pragma unroll
    for (int k = 0; k < np; ++k)
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
    __shared__ double part[EPG_BLOCK / 64][np];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < np; ++k) part[wave][k] = acc[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < np) {
        double s = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < EPG_BLOCK / 64; ++w) s += part[w][threadIdx.x];
        ws[(long)blockIdx.x * EPG_ROW + threadIdx.x] = s;
    }
}

template <typename real>
__global__ __launch_bounds__(64) void env_param_grad_final_kernel(const double *__restrict__ ws, int rows, int np, real *__restrict__ out)
{
    const int lane = threadIdx.x;
    for (int k = 0; k < np; ++k) {
        double s = 0;
        for (int r = lane; r < rows; r += 64) s += ws[(long)r * EPG_ROW + k];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) out[k] = (real)s;
    }
}

// rows of the workspace = blocks of the first kernel
static int64_t env_param_grad_rows(int64_t N)
{
    const int64_t blocks = (N + EPG_BLOCK - 1) / EPG_BLOCK;
    return blocks < 1 ? 1 : (blocks > EPG_MAX_BLOCKS ? EPG_MAX_BLOCKS : blocks);
}

int64_t env_param_grad_workspace_bytes(int64_t N) { return env_param_grad_rows(N) * EPG_ROW * (int64_t)sizeof(double); }

template <typename real>
int launch_env_param_grad(const EnvDesc<real> &env, long N, const real *x, const real *u, const real *gF, const real *gf,
                          real *gparams, double *ws, hipStream_t st)
{
    if (N <= 0) return MPC_OK;
    const int rows = (int)env_param_grad_rows(N);
    const dim3 grid((unsigned)rows), block(EPG_BLOCK);
    if (env.kind == MPC_ENV_PENDULUM)
        hipLaunchKernelGGL((env_param_grad_kernel<real, MPC_ENV_PENDULUM>), grid, block, 0, st, env, N, x, u, gF, gf, ws);
    else if (env.kind == MPC_ENV_PENDULUM_FULL)
        hipLaunchKernelGGL((env_param_grad_kernel<real, MPC_ENV_PENDULUM_FULL>), grid, block, 0, st, env, N, x, u, gF, gf, ws);
    else
        hipLaunchKernelGGL((env_param_grad_kernel<real, MPC_ENV_CARTPOLE>), grid, block, 0, st, env, N, x, u, gF, gf, ws);
    int rc = check_launch("env_param_grad_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(env_param_grad_final_kernel<real>, dim3(1), dim3(64), 0, st, ws, rows, env_np(env.kind), gparams);
    return check_launch("env_param_grad_final_kernel");
}

template int launch_env_param_grad<float>(const EnvDesc<float> &, long, const float *, const float *, const float *, const float *,
                                          float *, double *, hipStream_t);
template int launch_env_param_grad<double>(const EnvDesc<double> &, long, const double *, const double *, const double *,
                                           const double *, double *, double *, hipStream_t);

}  // namespace mpclqr
