// nn_dynamics64.hip -- mpc.dynamics.NNDynamics in float64 inside the kernels (mpc_mlp_*_dtype with MPC_F64, include/mpc_lqr.h 6d').
//
// What a float64 solve through a network needs from the device: lqr_forward through the network with the per-problem line search
// (mpc/lqr_step.py:164-261), util.get_traj / get_cost through it (mpc/util.py:102-153) and MPC.linearize_dynamics(ANALYTIC)
// (mpc/mpc.py:495-512).  A rollout is a chain of T dependent network evaluations per problem and trial: it is bound by latency,
// not by throughput, so the layers run on plain float64 FMA, ONE WAVEFRONT PER PROBLEM (per point), lanes across a layer's
// outputs -- no MFMA, no packed re-layout in global memory.  The arithmetic is csrc/nn_dynamics64.h, which a host build runs too.
//
// Memory: the network is nn.Linear's own tensors, copied into LDS by each block when it fits beside the wavefronts' areas
// (rows on an odd stride), else read in place through the caches.  The float32 kernels of nn_dynamics.hip are not touched.
// The workspace argument of the rollout and linearisation entries is checked like the float32 one (size, 16-byte alignment) and
// reserved: nothing reads or writes it today.
// The linearisation's weight gradient (mpc_mlp_param_grad_dtype, csrc/nn_param_grad64.h) is a BLOCK per point: nn64_param_grad_kernel
// keeps each thread's share of the sums in registers across its points and leaves one partial per block in the workspace,
// nn64_param_grad_final_kernel adds the partials in block order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <string>

#include "lqr_common.h"
#include "nn_dynamics64.h"
#include "nn_param_grad64.h"

namespace mpclqr {
namespace {

using nn64::Net;

// the wavefront as the executor of nn_dynamics64.h.  LDS instructions of one wavefront execute in order: only the compiler has
// to be kept from moving them (a wavefront's area is never touched by another wavefront)
struct WaveExec {
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ void sync() const { asm volatile("" ::: "memory"); }
    __device__ __forceinline__ double xor_get(double v, int mask) const { return __shfl_xor(v, mask); }
};

// grid: one wavefront per problem, blockDim.x / 64 problems per block
template <bool WL>
__global__ void __launch_bounds__(256) nn64_rollout_kernel(StepParams<double> p, Net arg, int wave_doubles)
{
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    __shared__ Net m;
    if (threadIdx.x == 0) m = arg;
    __syncthreads();
    if (WL) {
        nn64::stage_net(m, lds64, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    const long b = (long)blockIdx.x * nwave + wave;
    if (b >= p.B) return;
    WaveExec ex;
    nn64::rollout_problem<WL>(ex, p, m, lds64, lds64 + (WL ? m.total : 0) + (long)wave * wave_doubles, b);
}

// grid-stride over the points: a block stages the network once for all the points its wavefronts take
template <bool WL>
__global__ void __launch_bounds__(512) nn64_linearize_kernel(Net arg, long N, int ns, int nc, const double *x, const double *u, double *F,
                                                             double *f, int wave_doubles)
{
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    __shared__ Net m;
    if (threadIdx.x == 0) m = arg;
    __syncthreads();
    if (WL) {
        nn64::stage_net(m, lds64, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6, n = ns + nc;
    double *area = lds64 + (WL ? m.total : 0) + (long)wave * wave_doubles;
    WaveExec ex;
    for (long i = (long)blockIdx.x * nwave + wave; i < N; i += (long)gridDim.x * nwave)
        nn64::linearize_point<WL>(ex, m, lds64, area, ns, nc, x + i * ns, u + i * nc, F + i * ns * n, f + i * ns);
}

// the block as the executor of nn_param_grad64.h: the wavefront's lanes as above, the block's barrier
struct BlockExec {
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ double xor_get(double v, int mask) const { return __shfl_xor(v, mask); }
};

// grid-stride over the points, one point a block and pass; the block's sums leave as one partial (nn_param_grad64.h)
template <bool WL, int KMAX>
__global__ void __launch_bounds__(nn64::PG64_THREADS) nn64_param_grad_kernel(Net arg, nn64::GradLayout g, long N, int ns, int nc, const double *x,
                                                                             const double *u, const double *gF, const double *gf,
                                                                             double *partials)
{
    extern __shared__ __attribute__((aligned(16))) double lds64[];
    __shared__ Net m;
    if (threadIdx.x == 0) m = arg;
    __syncthreads();
    if (WL) {
        nn64::stage_net(m, lds64, threadIdx.x, blockDim.x);
        __syncthreads();
    }
    double acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
    double *area = lds64 + (WL ? m.total : 0);
    const long n = ns + nc;
    BlockExec ex;
    for (long i = blockIdx.x; i < N; i += gridDim.x)
        nn64::param_grad_point<WL, KMAX>(ex, m, g, lds64, area, x + i * ns, u + i * nc, gF + i * ns * n, gf + i * ns, acc);
    double *out = partials + (long)blockIdx.x * KMAX * nn64::PG64_THREADS;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) out[k * nn64::PG64_THREADS + threadIdx.x] = acc[k];
}

__global__ void __launch_bounds__(256) nn64_param_grad_final_kernel(nn64::GradFinal a, long entries)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < entries) nn64::sum_partials(a, e);
}

inline int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error((std::string(what) + ": " + hipGetErrorString(e)).c_str());
        return MPC_E_LAUNCH;
    }
    return MPC_OK;
}

struct Check { int code; const char *msg; };
int refuse(const Check &c) { set_last_error(c.msg); return c.code; }

constexpr int WIDTH_MAX = 4096;
constexpr int64_t WORKSPACE_BYTES = 256;
// (160 KiB a workgroup, less the kernels' static copy of the description)
constexpr size_t LDS_MAX = 160 * 1024 - 256, WEIGHTS_IN_LDS_MAX = 96 * 1024;

// the checks of a description, in the order and with the codes of the float32 entries (nn_dynamics.hip: mlp_check); `bind`: a
// call that will run (workspace, ctrl_carry, pointers), not a probe by widths
Check check_net(const mpc_mlp_dynamics *net, int ns, int nc, bool bind, const void *workspace, int64_t bytes)
{
    if (!net) return {MPC_E_NULL, "network is NULL"};
    const int L = net->n_layers;
    if (L < 1 || L > MPC_MLP_MAX_LAYERS) return {MPC_E_ARG, "network: 1..4 Linear layers"};
    if (bind && (net->activation < MPC_ACT_SIGMOID || net->activation > MPC_ACT_ELU)) return {MPC_E_ARG, "network: unknown activation"};
    if (net->widths[0] != ns + nc || net->widths[L] != ns) return {MPC_E_DIMS, "network: widths[0] must be n_state + n_ctrl, widths[L] n_state"};
    if (ns > 32) return {MPC_E_DIMS, "network kernels: n_state <= 32"};
    for (int l = 0; l <= L; ++l)
        if (net->widths[l] < 1 || net->widths[l] > WIDTH_MAX) return {MPC_E_DIMS, "network: layer width out of range"};
    if (!bind) return {MPC_OK, nullptr};
    if (WORKSPACE_BYTES > bytes || !workspace || ((uintptr_t)workspace & 15))
        return {MPC_E_ARG, "network: workspace too small or not 16-byte aligned (see mpc_mlp_workspace_bytes_dtype)"};
    if (net->ctrl_carry != 0 && net->ctrl_carry != nc) return {MPC_E_ARG, "network: ctrl_carry must be 0 or n_ctrl"};
    if (net->ctrl_carry >= ns) return {MPC_E_DIMS, "network: ctrl_carry needs n_state (augmented) > n_ctrl"};
    for (int l = 0; l < L; ++l)
        if (!net->W[l] || !net->b[l]) return {MPC_E_NULL, "network: weight / bias pointer is NULL"};
    return {MPC_OK, nullptr};
}

const Check TOO_WIDE = {MPC_E_DIMS, "network: layers too wide for the LDS-resident float64 kernel"};

void describe(const mpc_mlp_dynamics *net, Net &m)
{
    m.L = net->n_layers;
    m.act = net->activation;
    m.pass = net->passthrough ? 1 : 0;
    m.carry = net->ctrl_carry;
    for (int l = 0; l <= m.L; ++l) m.w[l] = net->widths[l];
    for (int l = 0; l < MPC_MLP_MAX_LAYERS; ++l) {
        m.W[l] = l < m.L ? (const double *)net->W[l] : nullptr;
        m.b[l] = l < m.L ? (const double *)net->b[l] : nullptr;
    }
    nn64::net_layout(m);
}

// What a launch does with a network: wavefronts per block, the network staged in LDS or not, the block's LDS
struct Plan {
    bool fits, wl;
    int nw, wave_doubles;
    size_t lds;
    unsigned grid;
};

Plan plan(const Net &m, bool jacobian, long items)
{
    Plan pl = {};
    const long wd = jacobian ? nn64::linearize_wave_doubles(m) : nn64::rollout_wave_doubles(m);
    const size_t wbytes = (size_t)m.total * 8, per_wave = (size_t)wd * 8;
    pl.wave_doubles = (int)wd;
    pl.wl = wbytes <= WEIGHTS_IN_LDS_MAX && wbytes + per_wave <= LDS_MAX;
    pl.fits = per_wave <= LDS_MAX;
    if (!pl.fits) return pl;
    // the linearisation streams many points through a block (eight wavefronts share one staged copy); a rollout is one long chain
    // per wavefront, four to a block
    pl.nw = jacobian ? 8 : 4;
    while (pl.nw > 1 && ((pl.wl ? wbytes : 0) + pl.nw * per_wave > LDS_MAX || (long)(pl.nw / 2) * 256 >= items)) pl.nw >>= 1;
    pl.lds = (pl.wl ? wbytes : 0) + pl.nw * per_wave;
    const long blocks = (items + pl.nw - 1) / pl.nw;
    pl.grid = (unsigned)(jacobian && blocks > 1024 ? 1024 : (blocks < 1 ? 1 : blocks));
    return pl;
}

// A kernel with dynamic LDS: past 64 KiB the runtime wants to be told -- once per kernel and device, raised to the budget's ceiling
// the first time a launch needs it (a pre-bound iteration launches these kernels every turn); a refusal is the call's error
template <auto Kernel, typename... A> int launch(const char *name, const Plan &pl, hipStream_t st, A... args)
{
    if (pl.lds > 64 * 1024) {
        static std::atomic<uint64_t> raised{0};
        int dev = 0;
        (void)hipGetDevice(&dev);
        const uint64_t bit = 1ull << (dev & 63);
        if (!(raised.load(std::memory_order_acquire) & bit)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
            if (e != hipSuccess) {
                set_last_error((std::string(name) + ": raising the dynamic LDS limit: " + hipGetErrorString(e)).c_str());
                return MPC_E_LAUNCH;
            }
            raised.fetch_or(bit, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(Kernel, dim3(pl.grid), dim3(64 * pl.nw), pl.lds, st, args...);
    return check_launch(name);
}

// The weight gradient's launch (nn_param_grad64.h): the KMAX instantiation that owns the network's weights and biases, the
// network staged beside the block's area or read in place.  fits == false: outside the kernel
struct GradPlan {
    bool fits, wl;
    int kmax;
    nn64::GradLayout g;
    size_t lds;
};

GradPlan grad_plan(const Net &m)
{
    GradPlan pl = {};
    pl.g = nn64::grad_layout(m);
    pl.kmax = nn64::grad_kmax(pl.g.entries);
    const size_t wbytes = (size_t)m.total * 8, area = (size_t)pl.g.doubles * 8;
    pl.fits = pl.kmax > 0 && area <= LDS_MAX;
    pl.wl = wbytes <= WEIGHTS_IN_LDS_MAX && wbytes + area <= LDS_MAX;
    pl.lds = (pl.wl ? wbytes : 0) + area;
    return pl;
}

inline long grad_blocks(long N) { return N < MPC_MLP_PARAM_GRAD64_MAX_BLOCKS ? N : MPC_MLP_PARAM_GRAD64_MAX_BLOCKS; }
// one partial of kmax * PG64_THREADS doubles a block (room for one at N = 0: the size never shrinks with N)
inline int64_t grad_workspace_bytes(const GradPlan &pl, long N)
{
    const long blocks = grad_blocks(N < 1 ? 1 : N);
    return (int64_t)blocks * pl.kmax * nn64::PG64_THREADS * 8;
}

// a complete description of a network the weight-gradient kernel takes (silent)
bool grad_describe(const mpc_mlp_dynamics *net, int ns, int nc, Net &m, GradPlan &pl)
{
    if (ns < 1 || nc < 1 || check_net(net, ns, nc, false, nullptr, 0).code) return false;
    if ((net->activation != MPC_ACT_SIGMOID && net->activation != MPC_ACT_RELU) || net->ctrl_carry != 0) return false;
    for (int l = 0; l < net->n_layers; ++l)
        if (!net->W[l] || !net->b[l]) return false;
    describe(net, m);
    pl = grad_plan(m);
    return pl.fits;
}

template <bool WL, int KMAX, typename... A> int launch_grad(const GradPlan &pl, unsigned blocks, hipStream_t st, A... args)
{
    Plan lp = {};
    lp.lds = pl.lds;
    lp.nw = nn64::PG64_THREADS / 64;
    lp.grid = blocks;
    return launch<nn64_param_grad_kernel<WL, KMAX>>("nn64_param_grad_kernel", lp, st, args...);
}

}  // namespace

int64_t nn64_workspace_bytes(const mpc_mlp_dynamics *net)
{
    if (!net || net->n_layers < 1 || net->n_layers > MPC_MLP_MAX_LAYERS) return 0;
    return WORKSPACE_BYTES;
}

// bit 0: the rollout kernel takes this network, bit 1: the linearisation kernel.  By widths alone; silent.
int nn64_budget(const mpc_mlp_dynamics *net, int ns, int nc)
{
    if (ns < 1 || nc < 1 || check_net(net, ns, nc, false, nullptr, 0).code) return 0;
    Net m;
    describe(net, m);
    return (plan(m, false, 1).fits ? 1 : 0) | (plan(m, true, 1).fits ? 2 : 0);
}

int launch_nn64_rollout(const StepParams<double> &p, const mpc_mlp_dynamics *net, void *workspace, int64_t bytes, hipStream_t st)
{
    const Check c = check_net(net, p.ns, p.nc, true, workspace, bytes);
    if (c.code) return refuse(c);
    Net m;
    describe(net, m);
    const Plan pl = plan(m, false, p.B);
    if (!pl.fits) return refuse(TOO_WIDE);
    return pl.wl ? launch<nn64_rollout_kernel<true>>("nn64_rollout_kernel", pl, st, p, m, pl.wave_doubles)
                 : launch<nn64_rollout_kernel<false>>("nn64_rollout_kernel", pl, st, p, m, pl.wave_doubles);
}

int launch_nn64_linearize(const mpc_mlp_dynamics *net, long N, int ns, int nc, const double *x, const double *u, double *F, double *f,
                          void *workspace, int64_t bytes, hipStream_t st)
{
    if (net && net->ctrl_carry) return refuse({MPC_E_ARG, "mlp_linearize: ctrl_carry describes a rollout only (linearise the network itself)"});
    const Check c = check_net(net, ns, nc, true, workspace, bytes);
    if (c.code) return refuse(c);
    Net m;
    describe(net, m);
    const Plan pl = plan(m, true, N);
    if (!pl.fits) return refuse(TOO_WIDE);
    return pl.wl ? launch<nn64_linearize_kernel<true>>("nn64_linearize_kernel", pl, st, m, N, ns, nc, x, u, F, f, pl.wave_doubles)
                 : launch<nn64_linearize_kernel<false>>("nn64_linearize_kernel", pl, st, m, N, ns, nc, x, u, F, f, pl.wave_doubles);
}

int nn64_param_grad_supported(const mpc_mlp_dynamics *net, int ns, int nc)
{
    Net m;
    GradPlan pl;
    return grad_describe(net, ns, nc, m, pl) ? 1 : 0;
}

// -1: the network is outside the kernel
int64_t nn64_param_grad_workspace_bytes(const mpc_mlp_dynamics *net, int64_t N)
{
    if (!net || net->n_layers < 1 || net->n_layers > MPC_MLP_MAX_LAYERS) return -1;
    const int ns = net->widths[net->n_layers], nc = net->widths[0] - ns;
    Net m;
    GradPlan pl;
    if (!grad_describe(net, ns, nc, m, pl)) return -1;
    return grad_workspace_bytes(pl, N < 0 ? 0 : (long)N);
}

int launch_nn64_param_grad(const mpc_mlp_dynamics *net, long N, int ns, int nc, const double *x, const double *u, const double *gF,
                           const double *gf, const mpc_mlp_param_grads *out, void *workspace, int64_t bytes, hipStream_t st)
{
    // the checks, codes and order of launch_nn_param_grad (nn_dynamics.hip)
    if (net && net->ctrl_carry) return refuse({MPC_E_DIMS, "mlp_param_grad: ctrl_carry describes a rollout only (differentiate the network itself)"});
    if (net && net->activation == MPC_ACT_ELU) return refuse({MPC_E_DIMS, "mlp_param_grad: sigmoid and relu only (an ELU network keeps the module path)"});
    Check c = check_net(net, ns, nc, false, nullptr, 0);
    if (c.code) return refuse(c);
    if (net->activation < MPC_ACT_SIGMOID || net->activation > MPC_ACT_ELU) return refuse({MPC_E_ARG, "network: unknown activation"});
    Net m;
    GradPlan pl;
    if (!grad_describe(net, ns, nc, m, pl))
        return refuse({MPC_E_DIMS, "mlp_param_grad: the network is outside the float64 kernel (see mpc_mlp_param_grad_supported_dtype)"});
    if (bytes < grad_workspace_bytes(pl, N)) return refuse({MPC_E_DIMS, "mlp_param_grad: workspace too small (see mpc_mlp_param_grad_workspace_bytes_dtype)"});
    if ((uintptr_t)workspace & 15) return refuse({MPC_E_ARG, "mlp_param_grad: the workspace must be 16-byte aligned"});
    double *partials = static_cast<double *>(workspace);
    const long blocks = grad_blocks(N);
    if (blocks > 0) {
        int rc;
        const unsigned gr = (unsigned)blocks;
#define MPC_PG64_LAUNCH(WL, K) launch_grad<WL, K>(pl, gr, st, m, pl.g, N, ns, nc, x, u, gF, gf, partials)
        if (pl.kmax == nn64::PG64_KMAX_SMALL) rc = pl.wl ? MPC_PG64_LAUNCH(true, nn64::PG64_KMAX_SMALL) : MPC_PG64_LAUNCH(false, nn64::PG64_KMAX_SMALL);
        else if (pl.kmax == nn64::PG64_KMAX_MID) rc = pl.wl ? MPC_PG64_LAUNCH(true, nn64::PG64_KMAX_MID) : MPC_PG64_LAUNCH(false, nn64::PG64_KMAX_MID);
        else rc = pl.wl ? MPC_PG64_LAUNCH(true, nn64::PG64_KMAX_LARGE) : MPC_PG64_LAUNCH(false, nn64::PG64_KMAX_LARGE);
#undef MPC_PG64_LAUNCH
        if (rc) return rc;
    }
    nn64::GradFinal a = {};
    a.L = m.L;
    a.blocks = (int)blocks;
    a.stride = (long)pl.kmax * nn64::PG64_THREADS;
    a.partials = partials;
    for (int l = 0; l <= m.L; ++l) a.w[l] = m.w[l];
    for (int l = 0; l < m.L; ++l) {
        a.gW[l] = (double *)out->gW[l];
        a.gb[l] = (double *)out->gb[l];
    }
    hipLaunchKernelGGL(nn64_param_grad_final_kernel, dim3((unsigned)((pl.g.entries + 255) / 256)), dim3(256), 0, st, a, pl.g.entries);
    return check_launch("nn64_param_grad_final_kernel");
}

}  // namespace mpclqr
