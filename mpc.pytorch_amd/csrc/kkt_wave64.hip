// kkt_wave64.hip -- kkt_wave.hip's two kernels in float64: the closed-form part of LQRStepFn.backward (mpc/lqr_step.py:346-404) for
// float64 problems with 2 <= n = n_state + n_ctrl <= 64.  Forced only (mpc_lqr_kkt_grads_kernel, MPC_KKT_GRADS_WAVE64): kernel = 0
// keeps float64 on the generic kernel (lqr_generic.hip: one workgroup per problem, C and F restaged behind three barriers a timestep).
//
//   kkt_costate64_kernel   the two costate recursions (:355-385): one wavefront per problem, lane i owns state i and reads ROW i of C
//                          as given (an asymmetric C is a supported input, see kkt_wave.hip) and F column-wise; tau[j] / lam[m] reach
//                          the lanes as two 32-bit readlanes each; [C_t | F_t | record] arrive by LDS-DMA one timestep ahead, in
//                          a ring of two slots.  lam_{t+1}, dlam_{t+1} are parked in the first 2 n_state doubles of the dF_t block.
//   kkt_outer64_kernel     dC_t, dc_t, dF_t (:346-353, :387-400): one wavefront per (t, b), 16 bytes (two doubles) a lane, every output
//                          byte written exactly once by a non-temporal store (the block first picks its costates out of its dF_t block).
//
// Two forms of each, with the SAME arithmetic order (so a view moved off the 16-byte grid gives the same bits):
//   aligned   n and n_state even, every block and row on 16 bytes, even strides: 16 bytes a lane
//   general   everything else (8-byte alignment is all a double has): 4 bytes a lane -- global_load_lds has no 8-byte size, a double
//             is two dwords -- and pairs of outputs that may cross a row, the block's last element on its own
#include <string>
#include "lqr_common.h"

namespace mpclqr {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

#include "kkt_wave_dma.h"      // dma_block, dma_block4, wait_newer (shared with kkt_wave.hip)

__device__ __forceinline__ double lane_bcast(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

constexpr int REC_BYTES = 4 * 64 * 8;      // the record: four rows of 64 doubles -- tau* | dtau | c_x | dl_dx

// Two ring slots of [C_t | F_t | record]: stage t - 1 is in flight while timestep t is summed, behind vmcnt(0).  A third slot behind a
// counted wait, as kkt_wave.hip has it, measured within 3.5 % either way (12/4 slower, 13/4 and 32/8 faster: docs/history/r27.md) and a
// general-form stage of n = 64 is 262 instructions against vmcnt's 63, so there is none.  Every stage issues the same instructions,
// the stages past the end included; the record's general form is a row in two instructions of 64 dwords, the second one only where the
// row reaches its upper half (n resp. n_state > 32): an instruction is issued only where at least one lane takes part in it.
template <bool AL>
__global__ void __launch_bounds__(64) kkt_costate64_kernel(StepParams<double> p, const double *dx, const double *du,
                                                           const double *dl_dx, double *dF, double *df, double *dx_init)
{
    extern __shared__ __attribute__((aligned(16))) char kkt64_lds[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int ns = p.ns, nc = p.nc, n = ns + nc, T = p.T, B = p.B;
    const int cbytes = n * n * 8, fbytes = ns * n * 8, slot_bytes = cbytes + fbytes + REC_BYTES;
    const bool st = lane < ns;
    const int li = st ? lane : 0;
    // The record's lane -> source map.  Aligned: instruction k = 0, 1 carries rows 2 k + lane / 32, granule g = lane % 32 of 16 bytes.
    // General: instruction (q, h) carries dword 64 h + lane of row q, that is half `lane & 1` of element e = 32 h + lane / 2.
    constexpr int NSRC = AL ? 2 : 8;
    const char *rsrc[NSRC];
    long rstep[NSRC];                                             // bytes per timestep
#pragma unroll
    for (int k = 0; k < NSRC; ++k) {
        const int row = AL ? 2 * k + (lane >> 5) : k >> 1;
        const int e = AL ? 2 * (lane & 31) : 32 * (k & 1) + (lane >> 1);
        const double *src = nullptr;
        long step = 0;
        if (e < ns) {
            src = (row == 0 ? p.cur_x + (long)b * ns : row == 1 ? dx + (long)b * ns : row == 2 ? p.c + (long)b * p.c_sb : dl_dx + (long)b * ns) + e;
            step = row == 2 ? p.c_st : (long)B * ns;
        } else if (e < n && row < 2) {
            src = (row == 0 ? p.cur_u : du) + (long)b * nc + (e - ns);
            step = (long)B * nc;
        }
        rsrc[k] = src ? (const char *)src + (AL ? 0 : 4 * (lane & 1)) : nullptr;
        rstep[k] = step * 8;
    }
    auto issue = [&](int t, int slot) {
        t = t >= 0 ? t : 0;                                   // past the end: stage 0 again
        char *base = kkt64_lds + slot * slot_bytes;
        const double *Ct = p.C + (long)t * p.C_st + (long)b * p.C_sb;
        const double *Ft = T > 1 ? p.F + (long)(t < T - 1 ? t : T - 2) * p.F_st + (long)b * p.F_sb : nullptr;
        if (AL) {
            dma_block(Ct, base, cbytes, lane);
            if (T > 1) dma_block(Ft, base + cbytes, fbytes, lane);
#pragma unroll
            for (int k = 0; k < 2; ++k)          // (n_state >= 2: lane 0 of both instructions takes part)
                if (rsrc[k])
                    __builtin_amdgcn_global_load_lds((glb_void_t *)(rsrc[k] + (long)t * rstep[k]),
                                                     (lds_void_t *)(base + cbytes + fbytes + 1024 * k), 16, 0, 0);
        } else {
            dma_block4(Ct, base, cbytes, lane);
            if (T > 1) dma_block4(Ft, base + cbytes, fbytes, lane);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                // (wave-uniform: the upper half of a row is asked for only where somebody takes part in it)
                if ((k & 1) && (k < 4 ? n : ns) <= 32) continue;
                if (rsrc[k])
                    __builtin_amdgcn_global_load_lds((glb_void_t *)(rsrc[k] + (long)t * rstep[k]),
                                                     (lds_void_t *)(base + cbytes + fbytes + 256 * k), 4, 0, 0);
            }
        }
    };
    double lam = 0.0, dlam = 0.0;
    issue(T - 1, 0);
    int slot = 0;
    for (int t = T - 1; t >= 0; --t) {
        wait_newer(0);
        const double *Cl = (const double *)(kkt64_lds + slot * slot_bytes);
        const double *Fl = (const double *)(kkt64_lds + slot * slot_bytes + cbytes);
        const double *Rl = (const double *)(kkt64_lds + slot * slot_bytes + cbytes + fbytes);
        const double tau = lane < n ? Rl[lane] : 0.0, d = lane < n ? Rl[64 + lane] : 0.0;
        const double cc = st ? Rl[128 + lane] : 0.0, gx = st ? Rl[192 + lane] : 0.0;
        // the slot the PREVIOUS timestep worked on is free (its reads fed that timestep's sums): the next stage goes there
        issue(t - 1, slot ^ 1);
        const long tb = (long)t * B + b;
        double r1 = cc, r2 = -gx;
        // (C tau)[i], (C dtau)[i]: ROW i of C (mpc/lqr_step.py:355-383), the same order of sums in both forms
        if (AL) {
            for (int j = 0; j < n; j += 2) {
                const f64x2 cr = *(const f64x2 *)(Cl + li * n + j);
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    r1 = fma(cr[v], lane_bcast(tau, j + v), r1);
                    r2 = fma(cr[v], lane_bcast(d, j + v), r2);
                }
            }
        } else {
            for (int j = 0; j < n; ++j) {
                const double cr = Cl[li * n + j];
                r1 = fma(cr, lane_bcast(tau, j), r1);
                r2 = fma(cr, lane_bcast(d, j), r2);
            }
        }
        if (t < T - 1) {
            // (Fx' lam)[i] = sum_m F[m][i] lam[m]: consecutive lanes, consecutive doubles
            for (int m = 0; m < ns; ++m) {
                const double fm = Fl[m * n + li];
                r1 = fma(fm, lane_bcast(lam, m), r1);
                r2 = fma(fm, lane_bcast(dlam, m), r2);
            }
            if (st) {
                double *park = dF + tb * (long)(ns * n);
                park[lane] = lam;
                park[ns + lane] = dlam;
                if (df) df[tb * ns + lane] = -dlam;                               // :397-400
            }
        }
        lam = r1;
        dlam = r2;
        slot ^= 1;
    }
    if (st) dx_init[(long)b * ns + lane] = -dlam;                                 // :404
}

template <bool AL>
__global__ void __launch_bounds__(64) kkt_outer64_kernel(StepParams<double> p, const double *dx, const double *du, double *dC,
                                                         double *dc, double *dF)
{
    __shared__ __attribute__((aligned(16))) double sv[4][64];      // tau, dtau, lam_{t+1}, dlam_{t+1}
    const long tb = blockIdx.x;
    const int lane = threadIdx.x;
    const int ns = p.ns, nc = p.nc, n = ns + nc, T = p.T, B = p.B;
    const int t = (int)(tb / B);
    const bool have = t < T - 1;
    double tau = 0.0, d = 0.0;
    if (lane < ns) { tau = p.cur_x[tb * ns + lane]; d = dx[tb * ns + lane]; }
    else if (lane < n) { tau = p.cur_u[tb * nc + (lane - ns)]; d = du[tb * nc + (lane - ns)]; }
    sv[0][lane] = tau;
    sv[1][lane] = d;
    double *dFt = dF + tb * (long)(ns * n);
    if (have && lane < ns) {
        sv[2][lane] = dFt[lane];
        sv[3][lane] = dFt[ns + lane];
    }
    __syncthreads();
    if (lane < n) __builtin_nontemporal_store(-d, dc + tb * n + lane);                                         // :352-353
    // dC_t = -0.5 (dtau tau' + tau dtau')   (:346-351), two consecutive elements per lane
    double *dCt = dC + tb * (long)(n * n);
    for (int e = 2 * lane; e < n * n; e += 128) {
        int i = e / n, j = e - i * n;
        if (AL) {
            const double di = sv[1][i], ti = sv[0][i];
            const f64x2 tj = *(const f64x2 *)&sv[0][j], dj = *(const f64x2 *)&sv[1][j];
            f64x2 o;
#pragma unroll
            for (int v = 0; v < 2; ++v) o[v] = -0.5 * fma(di, tj[v], ti * dj[v]);
            __builtin_nontemporal_store(o, (f64x2 *)(dCt + e));
        } else {
            // any n: the pair may cross a row and the block starts on an 8-byte boundary only -- 16 bytes a lane all the same
            // (global memory takes unaligned vector stores), the block's last element on its own where n is odd
            f64x2 o;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int ii = i < n ? i : n - 1;
                o[v] = -0.5 * fma(sv[1][ii], sv[0][j], sv[0][ii] * sv[1][j]);
                if (++j == n) { j = 0; ++i; }
            }
            if (e + 2 <= n * n) __builtin_nontemporal_store(o, (f64x2_a8 *)(dCt + e));
            else __builtin_nontemporal_store(o[0], dCt + e);
        }
    }
    // dF_t = -(dlam_{t+1} tau' + lam_{t+1} dtau')   (:387-396)
    if (have) {
        for (int e = 2 * lane; e < ns * n; e += 128) {
            int i = e / n, j = e - i * n;
            if (AL) {
                const double li = sv[2][i], dli = sv[3][i];
                const f64x2 tj = *(const f64x2 *)&sv[0][j], dj = *(const f64x2 *)&sv[1][j];
                f64x2 o;
#pragma unroll
                for (int v = 0; v < 2; ++v) o[v] = -fma(dli, tj[v], li * dj[v]);
                __builtin_nontemporal_store(o, (f64x2 *)(dFt + e));
            } else {
                f64x2 o;
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const int ii = i < ns ? i : ns - 1;
                    o[v] = -fma(sv[3][ii], sv[0][j], sv[2][ii] * sv[1][j]);
                    if (++j == n) { j = 0; ++i; }
                }
                if (e + 2 <= ns * n) __builtin_nontemporal_store(o, (f64x2_a8 *)(dFt + e));
                else __builtin_nontemporal_store(o[0], dFt + e);
            }
        }
    }
}

// every block and row on the 16-byte grid: the aligned instantiations
bool wave64_aligned(const StepParams<double> &p, const double *dx, const double *du, const double *dl_dx, const double *dC, const double *dF)
{
    const int n = p.ns + p.nc;
    auto al = [](const void *q) { return ((uintptr_t)q & 15) == 0; };
    return n % 2 == 0 && p.ns % 2 == 0 && al(p.C) && (p.T == 1 || al(p.F)) && p.C_st % 2 == 0 && p.C_sb % 2 == 0 && p.F_st % 2 == 0 &&
           p.F_sb % 2 == 0 && al(p.c) && p.c_st % 2 == 0 && p.c_sb % 2 == 0 && al(p.cur_x) && al(p.cur_u) && al(dx) && al(du) && al(dl_dx) &&
           al(dC) && (p.T == 1 || al(dF));
}

template <bool AL>
void launch_costate64(const StepParams<double> &p, const double *dx, const double *du, const double *dl_dx, double *dF, double *df,
                      double *dx_init, hipStream_t st)
{
    // (n = 64, n_state = 63: 2 x ((4096 + 4032) x 8 + 2048) = 134,144 bytes of the CU's 160 KiB)
    const int n = p.ns + p.nc;
    const size_t lds = 2 * ((size_t)(n * n + p.ns * n) * 8 + REC_BYTES);
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&kkt_costate64_kernel<AL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kkt_costate64_kernel<AL>, dim3(p.B), dim3(64), lds, st, p, dx, du, dl_dx, dF, df, dx_init);
}

}  // namespace

bool kkt_wave64_sizes(int ns, int nc)
{
    return ns >= 1 && nc >= 1 && ns + nc <= 64;          // (n >= 2: the costates park in the first 2 n_state doubles of dF_t)
}

int launch_kkt_wave64(const StepParams<double> &p, const double *dx, const double *du, const double *dl_dx, double *dC,
                      double *dc, double *dF, double *df, double *dx_init, hipStream_t st)
{
    const bool al = wave64_aligned(p, dx, du, dl_dx, dC, dF);
    if (al) launch_costate64<true>(p, dx, du, dl_dx, dF, df, dx_init, st);
    else launch_costate64<false>(p, dx, du, dl_dx, dF, df, dx_init, st);
    if (al) hipLaunchKernelGGL(kkt_outer64_kernel<true>, dim3((unsigned)((long)p.T * p.B)), dim3(64), 0, st, p, dx, du, dC, dc, dF);
    else hipLaunchKernelGGL(kkt_outer64_kernel<false>, dim3((unsigned)((long)p.T * p.B)), dim3(64), 0, st, p, dx, du, dC, dc, dF);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error((std::string("kkt_wave64 kernels: ") + hipGetErrorString(e)).c_str());
        return MPC_E_LAUNCH;
    }
    return MPC_OK;
}

}  // namespace mpclqr
