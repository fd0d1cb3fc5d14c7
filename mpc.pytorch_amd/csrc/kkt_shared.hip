// kkt_shared.hip -- the closed-form part of LQRStepFn.backward (mpc/lqr_step.py:346-404) for a cost and a linear model that
// the whole batch SHARES: the gradients of C [T,n,n], c [T,n], F [T-1,ns,n], f [T-1,ns] are the sums over the batch of the
// per-problem outer products, and nothing per problem is written:
//
//     sum_b dC_t = -0.5 (D'X + X'D)          D = dtau_t [B,n],        X = tau*_t [B,n]
//     sum_b dc_t = -sum_b dtau_t
//     sum_b dF_t = -(dL'X + L'D)             L = lam_{t+1} [B,ns],    dL = dlam_{t+1} [B,ns]
//     sum_b df_t = -sum_b dlam_{t+1}
//
// a GEMM per timestep with the batch as the K dimension.  Three launches:
//   kkt_costate_kernel (kkt_wave.hip)   the two costate recursions, parked in a compact [T-1,B,2 ns] area of the workspace
//   kkt_shared_partial_kernel           v_mfma_f32_16x16x4_f32 over chunks of CH problems staged through LDS; block (t, q) takes
//                                       the chunks q, q + P, q + 2 P, ... of timestep t in that order and writes ONE partial
//   kkt_shared_finish_kernel            adds the P partials of a timestep in the order 0 .. P-1, symmetrises dC, applies the signs
// No atomics: the result is bitwise reproducible and depends on the prior contents of neither the outputs nor the workspace.
// P depends on (T, B) alone (kkt_shared_partials), never on the device.
#include <string>
#include "lqr_common.h"

namespace mpclqr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CH = 32;            // problems per staged chunk: eight MFMA k-steps

// words of one partial: D'X [n,n] | dL'X + L'D [ns,n] | sum D [n] | sum dL [ns]
__host__ __device__ inline long partial_words(int ns, int nc)
{
    const long n = ns + nc;
    return n * n + ns * n + n + ns;
}

// One chunk of two [B,w] arrays (rows of w contiguous floats, CH w < 8 NTHR of them) into columns col0 .. col0 + w - 1 of two LDS
// arrays [CH][S]: every load of the chunk is issued before the first store waits for one (a load-store pair per trip of a rolled
// loop costs one memory round trip per trip: 71 us for 45 MB at 12/4, T = 50, B = 4096).  Rows b >= nb are written as zeros.
template <int NTHR, int S>
__device__ __forceinline__ void stage_pair(const float *__restrict__ ga, const float *__restrict__ gb, float *sa, float *sb, int w, int col0,
                                           int nb, int tid)
{
    float va[8], vb[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = tid + q * NTHR;
        const bool in = e < nb * w;
        va[q] = in ? ga[e] : 0.f;
        vb[q] = in ? gb[e] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = tid + q * NTHR;
        if (e < CH * w) {
            const int b = e / w, i = e - b * w;
            sa[b * S + col0 + i] = va[q];
            sb[b * S + col0 + i] = vb[q];
        }
    }
}

// ... and the chunk's costates, rows [lam (ns) | dlam (ns)], into two LDS arrays (CH 2 ns < 16 NTHR words)
template <int NTHR, int S>
__device__ __forceinline__ void stage_costates(const float *__restrict__ g, float *sl, float *sm, int ns, int nb, int tid)
{
    float v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = tid + q * NTHR;
        v[q] = e < nb * 2 * ns ? g[e] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e = tid + q * NTHR;
        if (e < CH * 2 * ns) {
            const int b = e / (2 * ns), i = e - b * 2 * ns;
            if (i < ns) sl[b * S + i] = v[q];
            else sm[b * S + (i - ns)] = v[q];
        }
    }
}

// NT = tiles of 16 along n; NT wavefronts, wavefront w owns tile row w of D'X and (16 w < ns) of dL'X + L'D.
// LDS: four arrays [CH][S] (X, D, L, dL), S = 16, 48, 48, 80 words: S mod 32 = 16, so the two k-rows a ds_read_b32 lane group
// covers (lanes 0-15: problem k, lanes 16-31: problem k + 1, 16 consecutive words each) fall on disjoint halves of the 32 banks.
template <int NT>
__global__ void __launch_bounds__(64 * NT) kkt_shared_partial_kernel(const float *__restrict__ xs, const float *__restrict__ us,
                                                                      const float *__restrict__ dx, const float *__restrict__ du,
                                                                      const float *__restrict__ costates, float *__restrict__ partials,
                                                                      int T, int B, int ns, int nc, int P)
{
    constexpr int S = (NT | 1) * 16;
    constexpr int NTHR = 64 * NT;
    __shared__ float sX[CH * S], sD[CH * S], sL[CH * S], sM[CH * S];
    const int t = blockIdx.x / P, part = blockIdx.x - t * P;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = ns + nc;
    const bool have = t < T - 1;              // timestep T-1 has no dF, df
    const bool frow = have && 16 * w < ns;
    const int nchunks = (B + CH - 1) / CH;
    // the columns n .. 16 NT - 1 (and ns .. for the costates) are never written again: they stay zero
    for (int e = tid; e < CH * S; e += NTHR) {
        sX[e] = 0.f; sD[e] = 0.f; sL[e] = 0.f; sM[e] = 0.f;
    }
    f32x4 accC[NT], accF[NT];
    float sumD[NT], sumM = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        accC[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        accF[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        sumD[j] = 0.f;
    }
    for (int ch = part; ch < nchunks; ch += P) {
        const int b0 = ch * CH;
        const int nb = B - b0 < CH ? B - b0 : CH;
        const long rb = (long)t * B + b0;
        __syncthreads();                                          // the previous chunk's reads (first trip: the zero fill) are done
        // stage: rows b >= nb of the last chunk are zeros (the K dimension is padded to a multiple of four)
        stage_pair<NTHR, S>(xs + rb * ns, dx + rb * ns, sX, sD, ns, 0, nb, tid);
        stage_pair<NTHR, S>(us + rb * nc, du + rb * nc, sX, sD, nc, ns, nb, tid);
        if (have) stage_costates<NTHR, S>(costates + rb * 2 * ns, sL, sM, ns, nb, tid);
        __syncthreads();
        const int kend = (nb + 3) & ~3;
        for (int k0 = 0; k0 < kend; k0 += 4) {
            // A[i][k] and B[k][j] of the 16x16x4 form share one map: lane l holds (problem k0 + l / 16, column l % 16 of the tile)
            const int row = (k0 + (lane >> 4)) * S + (lane & 15);
            float fx[NT], fd[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                fx[j] = sX[row + 16 * j];
                fd[j] = sD[row + 16 * j];
            }
            const float da = sD[row + 16 * w];                    // (fd[w]: a run-time index into registers would go through scratch)
#pragma unroll
            for (int j = 0; j < NT; ++j) accC[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(da, fx[j], accC[j], 0, 0, 0);
            if (w == 0) {
#pragma unroll
                for (int j = 0; j < NT; ++j) sumD[j] += fd[j];
            }
            if (frow) {
                const float la = sL[row + 16 * w], ma = sM[row + 16 * w];
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    accF[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ma, fx[j], accF[j], 0, 0, 0);
                    accF[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(la, fd[j], accF[j], 0, 0, 0);
                }
                sumM += ma;
            }
        }
    }
    // the partial of (t, part).  C/D map of the 16x16 forms: register r of lane l is (row 4 (l / 16) + r, column l % 16)
    float *out = partials + ((long)t * P + part) * partial_words(ns, nc);
    const int col = lane & 15, r0 = 16 * w + 4 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int jj = 16 * j + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = r0 + r;
            if (i < n && jj < n) out[(long)i * n + jj] = accC[j][r];
            if (frow && i < ns && jj < n) out[(long)n * n + (long)i * n + jj] = accF[j][r];
        }
    }
    // column sums: the four k-rows of a lane's column sit 16 lanes apart
    float *od = out + (long)n * n + (long)ns * n;
    if (w == 0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float v = sumD[j];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lane < 16 && 16 * j + lane < n) od[16 * j + lane] = v;
        }
    }
    {
        float v = sumM;
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (frow && lane < 16 && 16 * w + lane < ns) od[n + 16 * w + lane] = v;
    }
}

// one thread per word of a timestep's partial: the P partials added in the order 0 .. P-1
__global__ void __launch_bounds__(256) kkt_shared_finish_kernel(const float *__restrict__ partials, float *sum_dC, float *sum_dc, float *sum_dF,
                                                                 float *sum_df, int T, int ns, int nc, int P)
{
    const int n = ns + nc;
    const long PS = partial_words(ns, nc);
    const int per_t = (int)((PS + 255) / 256);
    const int t = blockIdx.x / per_t;
    const long e = (long)(blockIdx.x - t * per_t) * 256 + threadIdx.x;
    if (e >= PS) return;
    const float *base = partials + (long)t * P * PS;
    const long nn = (long)n * n, nf = (long)ns * n;
    if (e < nn) {
        if (!sum_dC) return;
        const int i = (int)(e / n), j = (int)(e - (long)i * n);
        float a = 0.f, b = 0.f;
        for (int q = 0; q < P; ++q) {
            a += base[q * PS + e];
            b += base[q * PS + (long)j * n + i];
        }
        sum_dC[(long)t * nn + e] = -0.5f * (a + b);
        return;
    }
    float a = 0.f;
    if (e < nn + nf) {
        if (!sum_dF || t >= T - 1) return;
        for (int q = 0; q < P; ++q) a += base[q * PS + e];
        sum_dF[(long)t * nf + (e - nn)] = -a;
    } else if (e < nn + nf + n) {
        if (!sum_dc) return;
        for (int q = 0; q < P; ++q) a += base[q * PS + e];
        sum_dc[(long)t * n + (e - nn - nf)] = -a;
    } else {
        if (!sum_df || t >= T - 1) return;
        for (int q = 0; q < P; ++q) a += base[q * PS + e];
        sum_df[(long)t * ns + (e - nn - nf - n)] = -a;
    }
}

// bytes of the costate area in front of the partials, a multiple of 16
int64_t costate_bytes(int T, int B, int ns) { return (((int64_t)(T - 1) * B * 2 * ns * 4) + 15) & ~(int64_t)15; }

}  // namespace

// partials per timestep: enough blocks for about a thousand wavefronts' worth of timesteps x partials, at most one per chunk
// and at most MPC_KKT_SHARED_MAX_PARTIALS -- a function of (T, B) alone
int kkt_shared_partials(int T, int B)
{
    const int nchunks = (B + CH - 1) / CH;
    int P = (1024 + T - 1) / T;
    if (P > MPC_KKT_SHARED_MAX_PARTIALS) P = MPC_KKT_SHARED_MAX_PARTIALS;
    if (P > nchunks) P = nchunks;
    return P < 1 ? 1 : P;
}

int64_t kkt_shared_workspace_bytes(int T, int B, int ns, int nc)
{
    if (B <= 0) return 16;
    return costate_bytes(T, B, ns) + (int64_t)T * kkt_shared_partials(T, B) * partial_words(ns, nc) * 4;
}

int launch_kkt_shared(const StepParams<float> &p, const float *dx, const float *du, const float *dl_dx, float *sum_dC, float *sum_dc,
                      float *sum_dF, float *sum_df, float *dx_init, void *workspace, hipStream_t st)
{
    const int n = p.ns + p.nc, NT = (n + 15) / 16;
    float *costates = (float *)workspace;
    float *partials = (float *)((char *)workspace + costate_bytes(p.T, p.B, p.ns));
    int rc = launch_kkt_costates(p, dx, du, dl_dx, costates, dx_init, st);
    if (rc) return rc;
    if (!sum_dC && !sum_dc && !sum_dF && !sum_df) return MPC_OK;
    const int P = kkt_shared_partials(p.T, p.B);
    const dim3 grid((unsigned)((long)p.T * P));
#define MPC_KS(NT_) hipLaunchKernelGGL(kkt_shared_partial_kernel<NT_>, grid, dim3(64 * NT_), 0, st, p.cur_x, p.cur_u, dx, du, costates, partials, \
                                        p.T, p.B, p.ns, p.nc, P)
    switch (NT) {
    case 1: MPC_KS(1); break;
    case 2: MPC_KS(2); break;
    case 3: MPC_KS(3); break;
    default: MPC_KS(4); break;
    }
#undef MPC_KS
    const long PS = partial_words(p.ns, p.nc);
    hipLaunchKernelGGL(kkt_shared_finish_kernel, dim3((unsigned)(((PS + 255) / 256) * p.T)), dim3(256), 0, st, partials, sum_dC, sum_dc,
                       sum_dF, sum_df, p.T, p.ns, p.nc, P);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error((std::string("kkt_shared kernels: ") + hipGetErrorString(e)).c_str());
        return MPC_E_LAUNCH;
    }
    return MPC_OK;
}

}  // namespace mpclqr
