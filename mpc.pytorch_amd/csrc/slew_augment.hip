// slew_augment.hip -- the slew-rate augmentation of a QuadCost / LinDx problem (mpc/mpc.py:362-445) in ONE launch.
//
// With a slew_rate_penalty gamma the reference solves the same LQR step on the state z_t = (u_{t-1}, x_t), tau = (z, u):
//     aC = slew_C + pad(C)        slew_C: +gamma I on the (u_prev, u_prev) and (u, u) blocks, -gamma I on the two cross blocks
//     ac = [0; c]
//     aF = [[0 0 I], [0 F]]       row block 0 carries u_t into the next state's u_{t-1}
//     af = [0; f]
// None of it depends on the iterate, so a solve builds it once.  The torch composition is a zeros, four slice writes, a pad
// and five cats over [T,B,na,na]; here every output element is written exactly once by one grid-stride kernel.
//
// Stride 0 is preserved: an axis the input broadcasts (a shared [n,n] cost, `.expand()`ed by MPC._expand_cost) has extent 1
// in the output too -- one [na,na] block that stays L2-resident in the step kernels, not T*B copies of it.
//
// The only arithmetic is slew_C + pad(C), the add torch performs; +-gamma I and the identity of the carry block are stored.
#include "lqr_common.h"

namespace mpclqr {
namespace {

template <typename real>
struct SlewArgs {
    int ns, nc;
    real gamma;
    // input blocks and their T / B element strides; extents of the two leading axes of each OUTPUT (1 where the input's stride is 0)
    const real *C, *c, *F, *f;
    long C_st, C_sb, c_st, c_sb, F_st, F_sb, f_st, f_sb;
    long CeT, CeB, ceT, ceB, FeT, FeB, feT, feB;
    real *aC, *ac, *aF, *af;
    long nC, nc_, nF, nf;       // element counts of the four outputs
};

template <typename real>
__global__ void __launch_bounds__(256) slew_augment_kernel(SlewArgs<real> a)
{
    const int ns = a.ns, nc = a.nc, n = ns + nc, na = n + nc;
    const long total = a.nC + a.nc_ + a.nF + a.nf;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        long r = e;
        if (r < a.nC) {                                            // aC [CeT, CeB, na, na]
            const int j = (int)(r % na), i = (int)(r / na % na);
            const long blk = r / ((long)na * na), b = blk % a.CeB, t = blk / a.CeB;
            real s = 0;                                            // slew_C
            const bool ip = i < nc, iu = i >= n, jp = j < nc, ju = j >= n;
            if ((ip && jp && i == j) || (iu && ju && i == j)) s = a.gamma;
            else if ((ip && ju && j - n == i) || (iu && jp && i - n == j)) s = -a.gamma;
            real v = 0;                                            // pad(C, (nc, 0, nc, 0))
            if (!ip && !jp) v = a.C[t * a.C_st + b * a.C_sb + (long)(i - nc) * n + (j - nc)];
            a.aC[r] = s + v;
            continue;
        }
        r -= a.nC;
        if (r < a.nc_) {                                           // ac [ceT, ceB, na]
            const int i = (int)(r % na);
            const long blk = r / na, b = blk % a.ceB, t = blk / a.ceB;
            a.ac[r] = i < nc ? (real)0 : a.c[t * a.c_st + b * a.c_sb + (i - nc)];
            continue;
        }
        r -= a.nc_;
        if (r < a.nF) {                                            // aF [FeT, FeB, n, na]
            const int j = (int)(r % na), i = (int)(r / na % n);
            const long blk = r / ((long)na * n), b = blk % a.FeB, t = blk / a.FeB;
            real v;
            if (i < nc) v = j - n == i ? (real)1 : (real)0;        // the carry block (0 0 I)
            else if (j < nc) v = 0;
            else v = a.F[t * a.F_st + b * a.F_sb + (long)(i - nc) * n + (j - nc)];
            a.aF[r] = v;
            continue;
        }
        r -= a.nF;
        {                                                          // af [feT, feB, n]
            const int i = (int)(r % n);
            const long blk = r / n, b = blk % a.feB, t = blk / a.feB;
            a.af[r] = i < nc ? (real)0 : a.f[t * a.f_st + b * a.f_sb + (i - nc)];
        }
    }
}

}  // namespace

template <typename real>
int launch_slew_augment(const mpc_lqr_problem *p, double gamma, real *aC, real *ac, real *aF, real *af, hipStream_t st)
{
    SlewArgs<real> a;
    const long T = p->T, B = p->B, ns = p->ns, nc = p->nc, n = ns + nc, na = n + nc;
    a.ns = p->ns; a.nc = p->nc; a.gamma = (real)gamma;
    a.C = (const real *)p->C; a.c = (const real *)p->c; a.F = (const real *)p->F; a.f = (const real *)p->f;
    a.C_st = p->C_st; a.C_sb = p->C_sb; a.c_st = p->c_st; a.c_sb = p->c_sb;
    a.F_st = p->F_st; a.F_sb = p->F_sb; a.f_st = p->f_st; a.f_sb = p->f_sb;
    a.CeT = p->C_st ? T : 1; a.CeB = p->C_sb ? B : 1;
    a.ceT = p->c_st ? T : 1; a.ceB = p->c_sb ? B : 1;
    a.FeT = p->F_st ? T - 1 : (T > 1 ? 1 : 0); a.FeB = p->F_sb ? B : 1;
    a.feT = p->f_st ? T - 1 : (T > 1 ? 1 : 0); a.feB = p->f_sb ? B : 1;
    a.aC = aC; a.ac = ac; a.aF = aF; a.af = af;
    a.nC = a.CeT * a.CeB * na * na;
    a.nc_ = a.ceT * a.ceB * na;
    a.nF = (a.F && aF) ? a.FeT * a.FeB * n * na : 0;
    a.nf = (a.f && af) ? a.feT * a.feB * n : 0;
    const long total = a.nC + a.nc_ + a.nF + a.nf;
    long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(slew_augment_kernel<real>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error(hipGetErrorString(e));
        return MPC_E_LAUNCH;
    }
    return MPC_OK;
}
template int launch_slew_augment<float>(const mpc_lqr_problem *, double, float *, float *, float *, float *, hipStream_t);
template int launch_slew_augment<double>(const mpc_lqr_problem *, double, double *, double *, double *, double *, hipStream_t);

}  // namespace mpclqr
