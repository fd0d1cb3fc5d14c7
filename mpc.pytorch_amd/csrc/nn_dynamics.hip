// nn_dynamics.hip -- mpc.dynamics.NNDynamics (mpc/dynamics.py:15-128) inside the kernels, fp32.
//
// The reference calls the network from Python once per timestep per line-search pass (mpc/lqr_step.py:223-225,
// mpc/util.py:112-113) and builds its Jacobian with one [N, out, in] tensor per layer (mpc/dynamics.py:100-116).
// A fully connected network over a batch that shares its weights is a GEMM, so here a wavefront takes SIXTEEN
// problems (trajectory points) and runs every layer on v_mfma_f32_16x16x4_f32:
//
//   activations live as "features x problems": D[i][j] = z[feature 16 tile + i][problem j].  In the accumulator
//   layout lane (q, r) holds rows 4q..4q+3 of column r -- and with the contraction index of K-block v' taken as
//   feature 4q + v' that same register quadruple IS the B operand of the next layer (the contraction order of an
//   MFMA is free).  The A operand is the weight matrix as nn.Linear stores it: lane (q, r) reads
//   W[16 tile_out + r][16 tile_in + 4q .. +3], one 16-byte load for four MFMAs.  Nothing moves across lanes between
//   layers; activations go through LDS only to be indexable by a runtime tile number (registers are not).
//
//   nn_rollout_kernel    lqr_forward with the network as true_dynamics (mpc/lqr_step.py:164-261): per-problem feedback
//                        u' = K dx + u + alpha k, bounds, the quadratic cost and the per-problem line search around
//                        the shared-weight network; without gains it is util.get_traj / get_cost (mpc/util.py:102-153)
//   nn_linearize_kernel  MPC.linearize_dynamics(ANALYTIC) (mpc/mpc.py:495-512): F = d net / d [x;u] by the chain
//                        W_L diag(s_{L-1}) W_{L-1} ... diag(s_1) W_1 per point, every product after the first an MFMA
//                        whose B operand is the previous product's accumulator; f = net(x, u) - F [x;u]
//
// n_state <= 16 is one accumulator tile of output features; 16 < n_state <= 32 is two (nn_wide_rollout_kernel,
// nn_wide_linearize_kernel: the same bodies with the tile count ST = 2 -- lane (q, r) owns state features 16 s + 4q + v,
// s < ST; the second tile lives in registers, the LDS staging areas are the same).
//
// Weights are re-packed once per call into zero-padded [out_pad][in_pad] blocks (multiples of 16) in the workspace.
#include <string>
#include <type_traits>

#include "lqr_common.h"

namespace mpclqr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// The packed network: one block of floats, layer after layer, W_l as [wp[l+1]][wp[l] + 4] (rows padded by 16 bytes so
// that the sixteen rows a 16-byte-per-lane read touches do not fall on the same LDS banks) followed by b_l [wp[l+1]].
// The block is copied into LDS at kernel start when it fits (WL), else read from global memory through the caches.
struct MlpDesc {
    int L, act, pass;            // Linear layers, MPC_ACT_*, passthrough
    int carry;                   // mpc_mlp_dynamics.ctrl_carry
    int w[MPC_MLP_MAX_LAYERS + 1];   // widths: w[0] = n_state + n_ctrl, w[L] = n_state
    int wp[MPC_MLP_MAX_LAYERS + 1];  // rounded up to 16
    int woff[MPC_MLP_MAX_LAYERS], boff[MPC_MLP_MAX_LAYERS];   // offsets (floats) into the packed block
    int total;                   // floats in the packed block (a multiple of 4)
    const float *packed;         // in the workspace
};

struct PackArgs {
    MlpDesc d;
    const float *W[MPC_MLP_MAX_LAYERS], *b[MPC_MLP_MAX_LAYERS];
    float *dst;
};

__global__ void mlp_pack_kernel(PackArgs a)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    for (int l = 0; l < a.d.L; ++l) {
        const int in = a.d.w[l], out = a.d.w[l + 1], ldp = a.d.wp[l] + 4, outp = a.d.wp[l + 1];
        for (int e = tid; e < outp * ldp; e += nt) {
            const int o = e / ldp, i = e - o * ldp;
            a.dst[a.d.woff[l] + e] = (o < out && i < in) ? a.W[l][o * in + i] : 0.f;
        }
        for (int o = tid; o < outp; o += nt) a.dst[a.d.boff[l] + o] = o < out ? a.b[l][o] : 0.f;
    }
}

// wave-local ordering of LDS traffic: a wavefront's LDS instructions execute in order, only the compiler has to be
// kept from moving them (the per-wave staging areas are never touched by another wave)
__device__ __forceinline__ void wave_sync() { asm volatile("" ::: "memory"); }

// the activation on one accumulator (one wave-uniform branch per tile, not per element)
__device__ __forceinline__ f32x4 act_fn(f32x4 a, int kind)
{
    if (kind == MPC_ACT_SIGMOID) {
#pragma unroll
        for (int v = 0; v < 4; ++v) a[v] = __builtin_amdgcn_rcpf(1.f + __expf(-a[v]));   // v_exp_f32 + v_rcp_f32 (1 ulp each), no division sequence
    } else if (kind == MPC_ACT_RELU) {
#pragma unroll
        for (int v = 0; v < 4; ++v) a[v] = fmaxf(a[v], 0.f);
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) a[v] = a[v] > 0.f ? a[v] : expm1f(a[v]);   // F.elu, alpha = 1
    }
    return a;
}
// derivative of the activation from its OUTPUT (mpc/dynamics.py:104-112)
__device__ __forceinline__ f32x4 slope_fn(f32x4 z, int kind)
{
    if (kind == MPC_ACT_SIGMOID) {
#pragma unroll
        for (int v = 0; v < 4; ++v) z[v] = z[v] * (1.f - z[v]);
    } else if (kind == MPC_ACT_RELU) {
#pragma unroll
        for (int v = 0; v < 4; ++v) z[v] = z[v] > 0.f ? 1.f : 0.f;
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) z[v] = z[v] > 0.f ? 1.f : z[v] + 1.f;
    }
    return z;
}

// All layers for the sixteen columns staged in tauS (row r = column's [x;u], zero padded to wp[0]).  Hidden
// activations go to zbase: layer l at zbase + l * 16 * ZS when KEEP (the Jacobian needs them all), else ping-pong.
// Returns the output layer's accumulators: tile s holds features 16 s + 4q .. + 3 of column r (ST tiles: n_state <= 16 ST).
// wts: the packed network (LDS or global).  The operand loads of the next K-step are issued before the current
// one's MFMAs: with one wavefront per SIMD nothing else hides their latency.
template <int ST> struct OutTiles {
    f32x4 t[ST];
};

template <bool KEEP, int ST>
__device__ __forceinline__ OutTiles<ST> mlp_forward(const MlpDesc &m, const float *wts, const float *tauS, int TS, float *zbase,
                                                    int ZS, int q, int r)
{
    const float *in = tauS;
    int is = TS;
    OutTiles<ST> res;
#pragma unroll
    for (int s = 0; s < ST; ++s) res.t[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < m.L; ++l) {
        const int nin_t = m.wp[l] >> 4, nout_t = m.wp[l + 1] >> 4, ldp = m.wp[l] + 4;
        const float *W = wts + m.woff[l], *bias = wts + m.boff[l];
        float *dst = zbase + (KEEP ? l : (l & 1)) * 16 * ZS;
        const bool last = l + 1 == m.L;
        const float *irow = in + r * is + 4 * q;
        for (int to = 0; to < nout_t; ++to) {
            // four accumulation chains (one per K-block of a 16-byte load), joined at the end
            f32x4 a0 = *reinterpret_cast<const f32x4 *>(bias + 16 * to + 4 * q);
            f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
            const float *wrow = W + (16 * to + r) * ldp + 4 * q;
            f32x4 a = *reinterpret_cast<const f32x4 *>(wrow);
            f32x4 b = *reinterpret_cast<const f32x4 *>(irow);
            for (int ti = 0; ti < nin_t; ++ti) {
                const int nx = ti + 1 < nin_t ? ti + 1 : ti;
                const f32x4 an = *reinterpret_cast<const f32x4 *>(wrow + 16 * nx);
                const f32x4 bn = *reinterpret_cast<const f32x4 *>(irow + 16 * nx);
                a0 = mfma(a[0], b[0], a0);
                a1 = mfma(a[1], b[1], a1);
                a2 = mfma(a[2], b[2], a2);
                a3 = mfma(a[3], b[3], a3);
                a = an;
                b = bn;
            }
            f32x4 acc = (a0 + a1) + (a2 + a3);
            if (!last) {
                *reinterpret_cast<f32x4 *>(dst + r * ZS + 16 * to + 4 * q) = act_fn(acc, m.act);
            } else {
                // (a constant index per branch: a register array indexed by the loop counter would go to scratch memory)
                if (to == 0) res.t[0] = acc;
                if (ST > 1 && to == 1) res.t[ST - 1] = acc;
            }
        }
        wave_sync();
        in = dst;
        is = ZS;
    }
    return res;
}

// the packed network into LDS (all waves of the workgroup), or a pointer to it in global memory
template <bool WL> __device__ __forceinline__ const float *stage_weights(const MlpDesc &m, float *wl)
{
    if (!WL) return m.packed;
    for (int e = threadIdx.x * 4; e < m.total; e += blockDim.x * 4)
        *reinterpret_cast<f32x4 *>(wl + e) = *reinterpret_cast<const f32x4 *>(m.packed + e);
    __syncthreads();
    return wl;
}

// One row's share of J_t(tau') - J_t(tau_nominal) for the stage cost 0.5 tau'C tau + c'tau (mpc/lqr_step.py:230-232), any C:
//     0.5 tau''C tau' - 0.5 tb'C tb = 0.5 [ d'(C tau') + tb'(C d) ],   d = tau' - tb,
// from the row products s = (C tau')_i, s2 = (C d)_i, this row's tau'_i, d_i and c_i.  Round 5: the line search's test
// "did the cost get worse" (:176-179) was the comparison of two float32 sums of ~1e4 whose difference, from the third iLQR
// iteration on, is below their rounding (1e-2): a coin per trial and problem, and the unluckiest of the 16 problems of the
// unluckiest wavefront ran all ten trials -- 1.3 ms a rollout instead of 0.13 (profiles/r05_trace_nn_before.txt).  Every
// term here is proportional to d; the cost handed back is J(nominal) + this sum.
__device__ __forceinline__ float line_search_delta(float tau_i, float d_i, float s, float s2, float c_i)
{
    return fmaf(d_i, fmaf(0.5f, s, c_i), 0.5f * (tau_i - d_i) * s2);
}

// ---------------------------------------------------------------------------------------------------------------
// lqr_forward through the network (mpc/lqr_step.py:164-261), sixteen problems per wavefront.
// lane (q, r): problem r of the group, quarter q of every per-problem loop (controls i = q, q+4, ..; cost rows likewise);
// the state x' is the output accumulators: features 16 s + 4q .. + 3 of state tile s < ST (n_state <= 16 ST).
// ---------------------------------------------------------------------------------------------------------------
template <bool WL, int ST>
__device__ __forceinline__ void rollout_tiles(StepParams<float> p, MlpDesc m, int TS, int ZS, int wave_floats)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float *wts = stage_weights<WL>(m, lds);
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    float *tauS = lds + (WL ? m.total : 0) + wave * wave_floats, *dxS = tauS + 16 * TS, *zb = dxS + 16 * TS;
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const long group = (long)blockIdx.x * nwave + wave;
    if (group * 16 >= p.B) return;
    const long b_raw = group * 16 + r;
    const bool valid = b_raw < p.B;
    const long b = valid ? b_raw : p.B - 1;
    const int ns = p.ns, nc = p.nc, n = ns + nc, T = p.T;
    const long B = p.B;
    const bool has_gain = p.K != nullptr, has_cost = p.C != nullptr;
    const float old_cost = p.old_costs_in ? p.old_costs_in[b] : 0.f;
    for (int i = lane; i < 16 * TS; i += 64) {
        tauS[i] = 0.f;
        dxS[i] = 0.f;
    }
    wave_sync();
    float alpha = 1.f, cost = 0.f, dun = 0.f, full = 0.f;
    bool active = valid;
    const int max_ls = has_gain ? p.max_ls : 1;
    for (int pass = 0; pass < max_ls; ++pass) {
        float xr[ST][4];
#pragma unroll
        for (int s = 0; s < ST; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int f = 16 * s + 4 * q + v;
                xr[s][v] = f < ns ? p.x_init[b * ns + f] : 0.f;
                if (active && f < ns) p.new_x[b * ns + f] = xr[s][v];
            }
        float ca = 0.f, da = 0.f;
        for (int t = 0; t < T; ++t) {
            const long tb = (long)t * B + b;
#pragma unroll
            for (int s = 0; s < ST; ++s)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int f = 16 * s + 4 * q + v;
                    if (f < ns) {
                        tauS[r * TS + f] = xr[s][v];
                        dxS[r * TS + f] = has_gain ? xr[s][v] - p.cur_x[tb * ns + f] : 0.f;   // :227
                    }
                }
            wave_sync();
            for (int i = q; i < nc; i += 4) {
                const float u = p.cur_u[tb * nc + i];
                float un = u;
                if (has_gain) {
                    const float *Kr = p.K + (tb * nc + i) * ns;
                    float s = 0.f;
                    for (int j = 0; j < ns; ++j) s = fmaf(Kr[j], dxS[r * TS + j], s);
                    // (dx_0 = 0 whatever current_x[0] is, :182; dxS keeps tau' - tau_nominal for the cost difference below)
                    un = (t == 0 ? 0.f : s) + u + alpha * p.k[tb * nc + i];                 // :192
                    if (p.zero_mask && p.zero_mask[tb * nc + i]) un = 0.f;                  // :197-198
                    if (p.bound_mode != MPC_BOUND_NONE) {                                   // :200-213
                        float lo = p.bound_mode == MPC_BOUND_SCALAR ? p.lo_s : p.lo[tb * nc + i];
                        float hi = p.bound_mode == MPC_BOUND_SCALAR ? p.hi_s : p.hi[tb * nc + i];
                        if (p.has_delta) {
                            const float l2 = u - p.delta_u, h2 = u + p.delta_u;
                            lo = (l2 < lo) ? lo : l2;
                            hi = (h2 > hi) ? hi : h2;
                        }
                        if (un < lo) un = lo;                                               // util.eclamp
                        if (un > hi) un = hi;
                    }
                    if (active) p.new_u[tb * nc + i] = un;
                }
                tauS[r * TS + ns + i] = un;
                const float d = u - un;
                dxS[r * TS + ns + i] = -d;          // (the control part of tau' - tau_nominal, for the cost difference below; K reads states only)
                da = fmaf(d, d, da);
            }
            wave_sync();
            if (has_cost) {                                                                 // :230-232
                const float *Ct = p.C + (long)t * p.C_st + b * p.C_sb;
                const float *ct = p.c + (long)t * p.c_st + b * p.c_sb;
                for (int i = q; i < n; i += 4) {
                    float s = 0.f, s2 = 0.f;
                    for (int j = 0; j < n; ++j) {
                        const float cij = Ct[i * n + j];
                        s = fmaf(cij, tauS[r * TS + j], s);
                        if (has_gain) s2 = fmaf(cij, dxS[r * TS + j], s2);
                    }
                    if (has_gain) {
                        // the line search compares J(tau') with J(nominal) (:176-179): summed as their DIFFERENCE, see line_search_delta
                        ca += line_search_delta(tauS[r * TS + i], dxS[r * TS + i], s, s2, ct[i]);
                    } else {
                        ca = fmaf(tauS[r * TS + i], fmaf(0.5f, s, ct[i]), ca);
                    }
                }
            }
            if (t < T - 1) {                                                                // :223-225
                const OutTiles<ST> o = mlp_forward<false, ST>(m, wts, tauS, TS, zb, ZS, q, r);
#pragma unroll
                for (int s = 0; s < ST; ++s)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int f = 16 * s + 4 * q + v;
                        // mpc/dynamics.py:74-75; an augmented state's first entries are the control just applied (:139-147)
                        const float skip = f < m.carry ? tauS[r * TS + ns + f] : (m.pass ? xr[s][v] : 0.f);
                        xr[s][v] = f < ns ? o.t[s][v] + skip : 0.f;
                        if (active && f < ns) p.new_x[((long)(t + 1) * B + b) * ns + f] = xr[s][v];
                    }
                wave_sync();
            } else {
                wave_sync();
            }
        }
        ca += __shfl_xor(ca, 16);
        ca += __shfl_xor(ca, 32);
        da += __shfl_xor(da, 16);
        da += __shfl_xor(da, 32);
        const float dn = sqrtf(da);
        if (pass == 0) full = dn;                                                           // :243-245
        if (active) {
            cost = has_gain ? old_cost + ca : ca;       // (with gains `ca` is J(tau') - J(nominal))
            dun = dn;
            // :176-179, 247: keep shrinking while this problem's cost got worse
            if (has_gain && ca > 0.f && pass + 1 < max_ls) alpha *= p.ls_decay; else active = false;
        }
        if (!__any(active)) break;
    }
    if (q == 0 && valid) {
        if (p.costs) p.costs[b] = cost;
        if (p.old_costs) p.old_costs[b] = old_cost;
        if (p.full_du_norm) p.full_du_norm[b] = full;
        if (p.alpha_du_norm) p.alpha_du_norm[b] = dun;
        if (p.alphas) p.alphas[b] = alpha;
        if (p.status && (!(cost == cost) || fabsf(cost) > 3e38f)) p.status[b] |= MPC_ST_NONFINITE;
    }
}

template <bool WL>
__global__ void __launch_bounds__(256) nn_rollout_kernel(StepParams<float> p, MlpDesc m, int TS, int ZS, int wave_floats)
{
    rollout_tiles<WL, 1>(p, m, TS, ZS, wave_floats);
}
// 16 < n_state <= 32: two state tiles, the second one in registers next to the first (same LDS staging, same launch)
template <bool WL>
__global__ void __launch_bounds__(256) nn_wide_rollout_kernel(StepParams<float> p, MlpDesc m, int TS, int ZS, int wave_floats)
{
    rollout_tiles<WL, 2>(p, m, TS, ZS, wave_floats);
}

// Where a linearisation reads x and writes (F, f), in floats -- launch parameters, so that the layout of the slew-rate
// augmentation (mpc_mlp_linearize_carry: state (u_prev, x), aF = [[0 0 I], [0 F]], af = [0; f]) runs the arithmetic of the dense one
// (mpc_mlp_linearize) instruction for instruction; only addresses differ.
struct LinLayout {
    int xs, xo;         // x of point p: x + p xs + xo
    int Fp, Fr, Fo;     // F[i][j] of point p: F + p Fp + Fo + i Fr + j
    int fs, fo;         // f[i] of point p: f + p fs + fo
    int carry;          // 0: dense.  n_ctrl: the augmented layout -- the constant blocks are written too (below), and a network row's
                        // store also zeroes the `carry` floats in front of it (the u_prev columns: Fo = carry Fr + carry)
};
inline LinLayout dense_layout(int ns, int nc) { return LinLayout{ns, 0, ns * (ns + nc), ns + nc, 0, ns, 0, 0}; }
inline LinLayout carry_layout(int ns, int nc)
{
    const int na = ns + nc, W = na + nc;
    return LinLayout{na, nc, na * W, W, nc * W + nc, na, nc, nc};
}

// The constant blocks of the augmented layout, by each wavefront for its own sixteen points: a point's carry rows are ONE contiguous run
// of carry (na + carry) floats at the head of its matrix, element (i, j) = (j == na + i); af starts with `carry` zeros.
__device__ __forceinline__ void write_carry_blocks(const LinLayout &lay, long p0, long N, int ns, float *F, float *f, int lane)
{
    const int nc = lay.carry, W = lay.Fr, na = ns + nc, run = nc * W;
    const int np = (int)(N - p0 < 16 ? N - p0 : 16);
    for (int e = lane; e < run; e += 64) {
        const int i = e / W, j = e - i * W;
        const float v = j == na + i ? 1.f : 0.f;
        for (int pp = 0; pp < np; ++pp) F[(p0 + pp) * lay.Fp + e] = v;
    }
    for (int e = lane; e < np * nc; e += 64) {
        const int pp = e / nc, i = e - pp * nc;
        f[(p0 + pp) * lay.fs + i] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// F = d net / d [x;u], f = net(x, u) - F [x;u] at N points (mpc/mpc.py:495-512 + mpc/dynamics.py:82-128), sixteen
// points per wavefront: one forward pass for all sixteen, then the chain of one point at a time.  A product
// G_l = diag(s_l) W_l G_{l-1} is [width_l x n]: tile (to, tj) in accumulator layout is rows 16 to + 4q + v, column
// 16 tj + r -- written to this lane's own LDS slot and read back by this lane as the B operand of layer l + 1.
// ---------------------------------------------------------------------------------------------------------------
// ST: row tiles of the output layer (n_state <= 16 ST).
template <bool WL, int ST>
__device__ __forceinline__ void linearize_tiles(MlpDesc m, long N, int ns, int nc, const float *x, const float *u,
                                                float *F, float *f, LinLayout lay, int TS, int ZS, int GT, int wave_floats)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float *wts = stage_weights<WL>(m, lds);
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    float *tauS = lds + (WL ? m.total : 0) + wave * wave_floats, *zb = tauS + 16 * TS;
    f32x4 *G0 = reinterpret_cast<f32x4 *>(zb + (m.L > 1 ? m.L - 1 : 1) * 16 * ZS), *G1 = G0 + GT * 64;
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const long p0 = ((long)blockIdx.x * nwave + wave) * 16;
    if (p0 >= N) return;
    const long pt = (p0 + r < N) ? p0 + r : N - 1;
    const int n = ns + nc, NTJ = m.wp[0] >> 4;
    if (lay.carry) write_carry_blocks(lay, p0, N, ns, F, f, lane);
    for (int f0 = 4 * q; f0 < m.wp[0]; f0 += 16) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int fe = f0 + v;
            tauS[r * TS + fe] = fe < ns ? x[pt * lay.xs + lay.xo + fe] : (fe < n ? u[pt * nc + (fe - ns)] : 0.f);
        }
    }
    wave_sync();
    OutTiles<ST> out = mlp_forward<true, ST>(m, wts, tauS, TS, zb, ZS, q, r);
    if (m.pass) {
#pragma unroll
        for (int s = 0; s < ST; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) out.t[s][v] += (16 * s + 4 * q + v < ns) ? tauS[r * TS + 16 * s + 4 * q + v] : 0.f;
    }
    const int Lh = m.L - 1;
    for (int pp = 0; pp < 16; ++pp) {
        if (p0 + pp >= N) break;
        f32x4 *Gprev = G0, *Gcur = G1;
        for (int l = 0; l < Lh; ++l) {
            const int nout_t = m.wp[l + 1] >> 4, nin_t = m.wp[l] >> 4, ld = m.wp[l] + 4;
            const float *zrow = zb + l * 16 * ZS + pp * ZS;
            const float *W = wts + m.woff[l];
            for (int to = 0; to < nout_t; ++to) {
                const f32x4 s = slope_fn(*reinterpret_cast<const f32x4 *>(zrow + 16 * to + 4 * q), m.act);
                for (int tj = 0; tj < NTJ; ++tj) {
                    f32x4 g;
                    if (l == 0) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) g[v] = s[v] * W[(16 * to + 4 * q + v) * ld + 16 * tj + r];
                    } else {
                        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
                        const float *wrow = W + (16 * to + r) * ld + 4 * q;
                        for (int ti = 0; ti < nin_t; ++ti) {
                            const f32x4 a = *reinterpret_cast<const f32x4 *>(wrow + 16 * ti);
                            const f32x4 gp = Gprev[(ti * NTJ + tj) * 64 + lane];
                            a0 = mfma(a[0], gp[0], a0);
                            a1 = mfma(a[1], gp[1], a1);
                            a2 = mfma(a[2], gp[2], a2);
                            a3 = mfma(a[3], gp[3], a3);
                        }
                        g = ((a0 + a1) + (a2 + a3)) * s;
                    }
                    Gcur[(to * NTJ + tj) * 64 + lane] = g;
                }
            }
            f32x4 *sw = Gprev;
            Gprev = Gcur;
            Gcur = sw;
        }
        // output layer: J = W_L G_{L-1}, ST row tiles side by side (one read of G_{L-1} feeds them all)
        float fs[ST][4];
#pragma unroll
        for (int s = 0; s < ST; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) fs[s][v] = 0.f;
        float *Fb = F + (p0 + pp) * lay.Fp + lay.Fo;
        {
            const int l = Lh, nin_t = m.wp[l] >> 4, ld = m.wp[l] + 4;
            const float *W = wts + m.woff[l];
            for (int tj = 0; tj < NTJ; ++tj) {
                f32x4 J[ST];
                if (Lh == 0) {
#pragma unroll
                    for (int s = 0; s < ST; ++s)
#pragma unroll
                        for (int v = 0; v < 4; ++v) J[s][v] = W[(16 * s + 4 * q + v) * ld + 16 * tj + r];
                } else {
                    f32x4 a0[ST], a1[ST], a2[ST], a3[ST];
#pragma unroll
                    for (int s = 0; s < ST; ++s) a0[s] = a1[s] = a2[s] = a3[s] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const float *wrow = W + r * ld + 4 * q;
                    for (int ti = 0; ti < nin_t; ++ti) {
                        f32x4 a[ST];
#pragma unroll
                        for (int s = 0; s < ST; ++s) a[s] = *reinterpret_cast<const f32x4 *>(wrow + 16 * s * ld + 16 * ti);
                        const f32x4 gp = Gprev[(ti * NTJ + tj) * 64 + lane];
#pragma unroll
                        for (int s = 0; s < ST; ++s) {
                            a0[s] = mfma(a[s][0], gp[0], a0[s]);
                            a1[s] = mfma(a[s][1], gp[1], a1[s]);
                            a2[s] = mfma(a[s][2], gp[2], a2[s]);
                            a3[s] = mfma(a[s][3], gp[3], a3[s]);
                        }
                    }
#pragma unroll
                    for (int s = 0; s < ST; ++s) J[s] = (a0[s] + a1[s]) + (a2[s] + a3[s]);
                }
                const int j = 16 * tj + r;
                const float tj_tau = tauS[pp * TS + j];
#pragma unroll
                for (int s = 0; s < ST; ++s)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int i = 16 * s + 4 * q + v;
                        if (m.pass && i == j && j < ns) J[s][v] += 1.f;                     // mpc/dynamics.py:118-125
                        if (i < ns && j < n) {
                            Fb[i * lay.Fr + j] = J[s][v];
                            if (j < lay.carry) Fb[i * lay.Fr + j - lay.carry] = 0.f;        // (the u_prev columns of this row)
                        }
                        fs[s][v] = fmaf(J[s][v], tj_tau, fs[s][v]);
                    }
            }
        }
#pragma unroll
        for (int s = 0; s < ST; ++s)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float a = fs[s][v];
                a += __shfl_xor(a, 1);
                a += __shfl_xor(a, 2);
                a += __shfl_xor(a, 4);
                a += __shfl_xor(a, 8);
                fs[s][v] = a;
            }
        if (r == pp) {
#pragma unroll
            for (int s = 0; s < ST; ++s)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int i = 16 * s + 4 * q + v;
                    if (i < ns) f[(p0 + pp) * lay.fs + lay.fo + i] = out.t[s][v] - fs[s][v];   // mpc/mpc.py:508-509
                }
        }
    }
}

template <bool WL>
__global__ void __launch_bounds__(512) nn_linearize_kernel(MlpDesc m, long N, int ns, int nc, const float *x, const float *u,
                                                           float *F, float *f, LinLayout lay, int TS, int ZS, int GT, int wave_floats)
{
    linearize_tiles<WL, 1>(m, N, ns, nc, x, u, F, f, lay, TS, ZS, GT, wave_floats);
}
// 16 < n_state <= 32: two row tiles of the output layer, of F and of f
template <bool WL>
__global__ void __launch_bounds__(512) nn_wide_linearize_kernel(MlpDesc m, long N, int ns, int nc, const float *x, const float *u,
                                                                float *F, float *f, LinLayout lay, int TS, int ZS, int GT, int wave_floats)
{
    linearize_tiles<WL, 2>(m, N, ns, nc, x, u, F, f, lay, TS, ZS, GT, wave_floats);
}

// ===============================================================================================================
// The network the reference builds by default -- ONE hidden layer (mpc/dynamics.py:16: hidden_sizes=[100]) -- with
// n_state + n_ctrl <= 16 and at most 16 HT hidden units: the whole network lives in registers.  A operands of both
// layers, the biases and (for the Jacobian) W_1 in accumulator layout are loaded once per wavefront; the hidden
// activations never leave the accumulators (tile `to` of layer 1's output IS K-step `to` of layer 2's B operand).
// ===============================================================================================================
template <int N> __device__ __forceinline__ float bcast(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x150 + N, 0xf, 0xf, true));   // row_newbcast:N
}

template <int HT> struct NetRegs {
    f32x4 w1[HT], b1[HT], w2[HT], b2;
};

template <int HT> __device__ __forceinline__ void load_net(NetRegs<HT> &R, const MlpDesc &m, int q, int r)
{
    const float *P = m.packed;
    const int ld2 = m.wp[1] + 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int to = 0; to < HT; ++to) {
        const bool in = 16 * to < m.wp[1];                      // (wave-uniform)
        const int tc = in ? to : 0;
        const f32x4 a = *reinterpret_cast<const f32x4 *>(P + m.woff[0] + (16 * tc + r) * 20 + 4 * q);
        const f32x4 bb = *reinterpret_cast<const f32x4 *>(P + m.boff[0] + 16 * tc + 4 * q);
        const f32x4 c = *reinterpret_cast<const f32x4 *>(P + m.woff[1] + r * ld2 + 16 * tc + 4 * q);
        R.w1[to] = in ? a : zero;
        R.b1[to] = in ? bb : zero;
        R.w2[to] = in ? c : zero;
    }
    R.b2 = *reinterpret_cast<const f32x4 *>(P + m.boff[1] + 4 * q);
}

// pre[to] = W_1 tau + b_1 (accumulator layout: hidden units 16 to + 4q + v, column r)
template <int HT> __device__ __forceinline__ void layer1(const NetRegs<HT> &R, f32x4 tq, f32x4 (&pre)[HT])
{
#pragma unroll
    for (int to = 0; to < HT; ++to) pre[to] = R.b1[to];
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
        for (int to = 0; to < HT; ++to) pre[to] = mfma(R.w1[to][v], tq[v], pre[to]);
}
// the same with layer 1's operands (A operand and bias of every tile) read from this lane's own LDS slots instead of
// 8 HT registers: the line-search kernel needs those registers for a timestep's rows of C and K
template <int HT> __device__ __forceinline__ void layer1_lds(const f32x4 *w1s, const f32x4 *b1s, f32x4 tq, f32x4 (&pre)[HT])
{
#pragma unroll
    for (int to = 0; to < HT; ++to) {
        const f32x4 w = w1s[64 * to];
        f32x4 a = b1s[64 * to];
#pragma unroll
        for (int v = 0; v < 4; ++v) a = mfma(w[v], tq[v], a);
        pre[to] = a;
    }
}
// W_2 z (+ init), four accumulation chains
template <int HT> __device__ __forceinline__ f32x4 layer2(const NetRegs<HT> &R, const f32x4 (&z)[HT], f32x4 init)
{
    f32x4 a0 = init, a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
#pragma unroll
    for (int to = 0; to < HT; ++to) {
        a0 = mfma(R.w2[to][0], z[to][0], a0);
        a1 = mfma(R.w2[to][1], z[to][1], a1);
        a2 = mfma(R.w2[to][2], z[to][2], a2);
        a3 = mfma(R.w2[to][3], z[to][3], a3);
    }
    return (a0 + a1) + (a2 + a3);
}

// sixteen floats of a row that need not be 16-byte aligned or 16 long (columns >= len come back as 0).  Every load is
// unconditional from a clamped address and masked afterwards: a load under a lane-dependent condition becomes a branch
// around it, and the joins of those branches are where the compiler drains the whole load queue.
__device__ __forceinline__ void load_row(const float *row, int len, bool vec, f32x4 (&o)[4])
{
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (vec) {
            const bool in = 4 * g < len;
            const f32x4 t = *reinterpret_cast<const f32x4 *>(row + (in ? 4 * g : 0));
            o[g] = in ? t : f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = 4 * g + e < len;
                const float t = row[in ? 4 * g + e : 0];
                o[g][e] = in ? t : 0.f;
            }
        }
    }
}
__device__ __forceinline__ float load_if(const float *p, long idx, bool in)
{
    const float t = p[in ? idx : 0];
    return in ? t : 0.f;
}

// lqr_forward through the network, one wavefront per workgroup, sixteen problems per wavefront (see nn_rollout_kernel
// for the roles of the lanes).  What one step needs from memory -- rows 4q..4q+3 of C_t, c_t, row q of K_t, k_t, the
// nominal -- is requested one step ahead, before the network's MFMAs, and consumed after them.
// GAIN: line search with feedback gains (else the controls are the nominal ones); COST: the quadratic cost is summed.
// Rows are read 16 bytes at a time: n_state and n_state + n_ctrl multiples of 4 (else the general kernel runs).
// ACT: the activation as a compile-time constant (the exp / reciprocal of 28 sigmoids per lane and step are the largest
// block of vector work in the step; a runtime switch keeps all three variants and their branches inside the time loop)
template <int HT, bool GAIN, bool COST, int ACT>
__global__ void __launch_bounds__(64) nn_rollout_fast_kernel(StepParams<float> p, MlpDesc m)
{
    __shared__ __attribute__((aligned(16))) float tauS[16 * 20], dxS[16 * 20];
    __shared__ f32x4 netS[GAIN && COST ? 2 * HT * 64 : 1];        // layer 1 of the line-search kernel: [w1 | b1][tile][lane]
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const long b_raw = (long)blockIdx.x * 16 + r;
    const bool valid = b_raw < p.B;
    const long b = valid ? b_raw : p.B - 1;
    const long b_raw_clamped = b;
    const int ns = p.ns, nc = p.nc, n = ns + nc, T = p.T;
    const long B = p.B;
    constexpr bool has_gain = GAIN, has_cost = COST, vecC = true, vecK = true;
    const float old_cost = p.old_costs_in ? p.old_costs_in[b] : 0.f;
    NetRegs<HT> R;
    load_net<HT>(R, m, q, r);
    for (int i = lane; i < 16 * 20; i += 64) {
        tauS[i] = 0.f;
        dxS[i] = 0.f;
    }
    if (GAIN && COST) {
        // (this instantiation sits at the 512-register limit: layer 1's operands move to LDS, two 16-byte reads per tile and step)
#pragma unroll
        for (int to = 0; to < HT; ++to) {
            netS[64 * to + lane] = R.w1[to];
            netS[64 * (HT + to) + lane] = R.b1[to];
            R.w1[to] = f32x4{0.f, 0.f, 0.f, 0.f};
            R.b1[to] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    wave_sync();
    float alpha = 1.f, cost = 0.f, dun = 0.f, full = 0.f;
    bool active = valid;
    const int max_ls = has_gain ? p.max_ls : 1;
    const bool own_u = q < nc;                  // this lane computes control i = q (n_ctrl <= 4)
    // The line search as a JOB SCHEDULE over the wave's sixteen problem slots (round 5).  The reference runs pass after pass over the
    // whole batch while any problem got worse (mpc/lqr_step.py:176-179); a wavefront did the same for its 16 problems -- and from the
    // third iLQR iteration on a few problems of most wavefronts need the 4th, 7th or 10th step size (tools/archive/r05_nn_iter_probe.py), so
    // the rollout of 0.14 ms ran 1.3 - 1.7 ms with one or two slots of sixteen at work (profiles/r05_trace_nn_before.txt).  The trials
    // of a problem do not depend on each other: after a pass, the slots nobody needs any more roll out FURTHER trials of the problems
    // that are still searching -- a problem's next S step sizes side by side, S = 16 / (problems searching) --, the first of them with
    // the stores on (as the sequential search would have it); a problem whose accepted trial is not the one in memory replays it
    // once.  Same step sizes (the same chain of float32 multiplications from 1), same acceptance rule -- the first trial that did not
    // get worse, else the last (:247-252) -- same results; three passes where the sequential search took up to max_ls.
    __shared__ int tabR[16], tabS[16];
    long bb = b;                                // the problem this lane's slot rolls out in the CURRENT pass
    float al = 1.f;                             // ... with this step size
    bool store = active;                        // ... writing new_x / new_u
    bool done_all = false;
    // the search state of this slot's OWN problem (what its q = 0 lane says counts; the other three carry copies)
    int next_t = 0, acc_t = -1, stored_t = -1;  // first trial not rolled out yet; the accepted one; the one whose trajectory is in memory
    bool done = !valid;
    // this pass's job of the slot, and where the own problem's jobs sit: slots [base, base + share), trials first_t ..
    int job_t = 0, base = r, share = valid ? 1 : 0, first_t = 0;
    bool job_valid = valid, replaying = false;
    auto chain = [&](int j) { float a = 1.f; for (int i = 0; i < j; ++i) a *= p.ls_decay; return a; };      // :247 alpha *= decay, j times
    auto schedule = [&]() {
        if (!done && acc_t < 0 && next_t >= max_ls) acc_t = max_ls - 1;                     // no trial improved: the last one stands (:250-252)
        const bool need_replay = !done && acc_t >= 0 && stored_t != acc_t;
        const bool searching = !done && acc_t < 0;
        const unsigned mR = (unsigned)__ballot(need_replay && q == 0), mS = (unsigned)__ballot(searching && q == 0);
        if ((mR | mS) == 0u) { done_all = true; return; }
        const int nR = __popc(mR), nS = __popc(mS), free_slots = 16 - nR;
        const int S = nS ? (free_slots >= nS ? free_slots / nS : 1) : 0;
        const unsigned below = (1u << r) - 1u;
        const int rankR = __popc(mR & below), rankS = __popc(mS & below);
        if (q == 0 && need_replay) tabR[rankR] = r;
        if (q == 0 && searching) tabS[rankS] = r;
        wave_sync();
        // the own problem's jobs of this pass
        replaying = need_replay;
        share = need_replay ? 1 : ((searching && rankS * S < free_slots) ? S : 0);
        base = need_replay ? rankR : nR + rankS * S;
        first_t = need_replay ? acc_t : next_t;
        // this slot's job
        const int k = r;
        int home = 0, off = 0;
        bool st = false;
        job_valid = false;
        if (k < nR) {
            home = tabR[k]; st = true; job_valid = true;
        } else if (S > 0 && (k - nR) / S < nS) {
            home = tabS[(k - nR) / S]; off = (k - nR) % S; st = off == 0; job_valid = true;
        }
        const int h_acc = __shfl(acc_t, home), h_next = __shfl(next_t, home);               // (lane `home`: q = 0 of that slot)
        job_t = (k < nR ? h_acc : h_next) + off;
        job_valid = job_valid && job_t < max_ls;
        bb = (long)__shfl((int)b_raw_clamped, home);
        al = chain(job_t);
        store = job_valid && st;
        wave_sync();
    };
    auto update_after_pass = [&](int pass, float ca, float dn) {
        if (!(GAIN && COST)) {                  // util.get_traj / get_cost: one pass, every slot its own problem
            cost = ca; dun = dn; full = dn; alpha = 1.f;
            done_all = true;
            return;
        }
        const unsigned ok = (unsigned)__ballot(q == 0 && job_valid && !(ca > 0.f));         // bit k: the trial in slot k did not get worse
        // the results of the own problem's first job (the one that stored) come from slot `base`
        const float ca0 = __shfl(ca, base), dn0 = __shfl(dn, base);
        if (!done && share > 0) {
            if (pass == 0) full = dn0;                                                      // :243-245 (trial 0 is alpha = 1)
            if (replaying) {
                cost = old_cost + ca0; dun = dn0; alpha = chain(acc_t);
                stored_t = acc_t; done = true;
            } else {
                const unsigned mine = (ok >> base) & ((1u << share) - 1u);
                const int n_run = min(share, max_ls - first_t);
                if (mine != 0u) acc_t = first_t + __ffs((int)mine) - 1;
                stored_t = first_t;
                next_t = first_t + n_run;
                // (what the sequential search would report had it stopped here: the trial in memory)
                cost = old_cost + ca0; dun = dn0; alpha = chain(first_t);
                if (acc_t < 0 && next_t >= max_ls) acc_t = max_ls - 1;
                if (acc_t == stored_t) done = true;
            }
        }
        schedule();
    };
    for (int pass = 0; ; ++pass) {
        const long b = bb;                      // (shadows the slot's own problem inside the pass)
        const float alpha = al;
        const bool active = store;
        f32x4 xr;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int f = 4 * q + v;
            xr[v] = load_if(p.x_init, b * ns + f, f < ns);
            if (active && f < ns) p.new_x[b * ns + f] = xr[v];
        }
        // operands of step t, requested one step ahead, before the network's MFMAs of step t - 1.  (Two steps ahead
        // with a second register set was no faster: at ~460 registers the loads serialise behind register reuse.)
        struct Ops {
            f32x4 Cr[4][4], Kr[4], cq, cx;
            float kq, uq;
        } opA;
        auto request = [&](int t, Ops &o) {
            const long tb = (long)t * B + b;
            if (has_cost) {
                const float *Ct = p.C + (long)t * p.C_st + b * p.C_sb, *ct = p.c + (long)t * p.c_st + b * p.c_sb;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int i = 4 * q + v < n ? 4 * q + v : 0;
                    load_row(Ct + i * n, 4 * q + v < n ? n : 0, vecC, o.Cr[v]);
                    o.cq[v] = load_if(ct, i, 4 * q + v < n);
                }
            }
            if (has_gain) {
                load_row(p.K + (tb * nc + (own_u ? q : 0)) * ns, own_u ? ns : 0, vecK, o.Kr);
                o.kq = load_if(p.k, tb * nc + q, own_u);
#pragma unroll
                for (int v = 0; v < 4; ++v) o.cx[v] = load_if(p.cur_x, tb * ns + 4 * q + v, 4 * q + v < ns);
            }
            o.uq = load_if(p.cur_u, tb * nc + q, own_u);
        };
        float ca = 0.f, da = 0.f;
        auto step = [&](int t, Ops &o) {
            const long tb = (long)t * B + b;
            // the state quad goes first: a quad that straddles n_state also covers control slots, written next
            *reinterpret_cast<f32x4 *>(tauS + r * 20 + 4 * q) = xr;
            *reinterpret_cast<f32x4 *>(dxS + r * 20 + 4 * q) = has_gain ? xr - o.cx : f32x4{0.f, 0.f, 0.f, 0.f};   // :227
            wave_sync();
            if (own_u) {
                const float uq = o.uq;
                float un = uq;
                if (has_gain) {
                    float s0 = 0.f, s1 = 0.f;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 d = *reinterpret_cast<const f32x4 *>(dxS + r * 20 + 4 * g);
                        s0 = fmaf(o.Kr[g][0], d[0], s0);
                        s1 = fmaf(o.Kr[g][1], d[1], s1);
                        s0 = fmaf(o.Kr[g][2], d[2], s0);
                        s1 = fmaf(o.Kr[g][3], d[3], s1);
                    }
                    // (dx_0 = 0 whatever current_x[0] is, :182; dxS keeps tau' - tau_nominal for the cost difference below)
                    un = (t == 0 ? 0.f : s0 + s1) + uq + alpha * o.kq;                      // :192
                    if (p.zero_mask && p.zero_mask[tb * nc + q]) un = 0.f;                  // :197-198
                    if (p.bound_mode != MPC_BOUND_NONE) {                                   // :200-213
                        float lo = p.bound_mode == MPC_BOUND_SCALAR ? p.lo_s : p.lo[tb * nc + q];
                        float hi = p.bound_mode == MPC_BOUND_SCALAR ? p.hi_s : p.hi[tb * nc + q];
                        if (p.has_delta) {
                            const float l2 = uq - p.delta_u, h2 = uq + p.delta_u;
                            lo = (l2 < lo) ? lo : l2;
                            hi = (h2 > hi) ? hi : h2;
                        }
                        if (un < lo) un = lo;                                               // util.eclamp
                        if (un > hi) un = hi;
                    }
                    if (active) p.new_u[tb * nc + q] = un;
                }
                tauS[r * 20 + ns + q] = un;
                const float d = uq - un;
                if (has_gain) dxS[r * 20 + ns + q] = -d;      // (the control part of tau' - tau_nominal; K's padded columns are zero)
                da = fmaf(d, d, da);
            }
            wave_sync();
            const f32x4 tq = *reinterpret_cast<const f32x4 *>(tauS + r * 20 + 4 * q);
            if (has_cost) {                                                                 // :230-232
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 tg = *reinterpret_cast<const f32x4 *>(tauS + r * 20 + 4 * g);
                    const f32x4 dg = has_gain ? *reinterpret_cast<const f32x4 *>(dxS + r * 20 + 4 * g) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int v = 0; v < 4; ++v)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            s[v] = fmaf(o.Cr[v][g][e], tg[e], s[v]);
                            if (has_gain) s2[v] = fmaf(o.Cr[v][g][e], dg[e], s2[v]);
                        }
                }
                if (has_gain) {
                    // J(tau') - J(nominal), summed as a difference (line_search_delta)
                    const f32x4 dq = *reinterpret_cast<const f32x4 *>(dxS + r * 20 + 4 * q);
#pragma unroll
                    for (int v = 0; v < 4; ++v) ca += line_search_delta(tq[v], dq[v], s[v], s2[v], o.cq[v]);
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v) ca = fmaf(tq[v], fmaf(0.5f, s[v], o.cq[v]), ca);
                }
            }
            if (t + 1 < T) request(t + 1, o);
            if (t + 1 < T) {
                f32x4 z[HT];                                                                // :223-225
                if (GAIN && COST) layer1_lds<HT>(netS + lane, netS + 64 * HT + lane, tq, z); else layer1<HT>(R, tq, z);
#pragma unroll
                for (int to = 0; to < HT; ++to) z[to] = act_fn(z[to], ACT);
                const f32x4 out = layer2<HT>(R, z, R.b2);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int f = 4 * q + v;
                    const float skip = f < m.carry ? tauS[r * 20 + ns + f] : (m.pass ? xr[v] : 0.f);   // mpc/dynamics.py:74-75, :139-147
                    xr[v] = f < ns ? out[v] + skip : 0.f;
                    if (active && f < ns) p.new_x[((long)(t + 1) * B + b) * ns + f] = xr[v];
                }
            }
            wave_sync();
        };
        request(0, opA);
        for (int t = 0; t < T; ++t) step(t, opA);
        ca += __shfl_xor(ca, 16);
        ca += __shfl_xor(ca, 32);
        da += __shfl_xor(da, 16);
        da += __shfl_xor(da, 32);
        const float dn = sqrtf(da);
        update_after_pass(pass, ca, dn);
        if (done_all) break;
    }
    if (q == 0 && valid) {
        if (p.costs) p.costs[b] = cost;
        if (p.old_costs) p.old_costs[b] = old_cost;
        if (p.full_du_norm) p.full_du_norm[b] = full;
        if (p.alpha_du_norm) p.alpha_du_norm[b] = dun;
        if (p.alphas) p.alphas[b] = alpha;
        if (p.status && (!(cost == cost) || fabsf(cost) > 3e38f)) p.status[b] |= MPC_ST_NONFINITE;
    }
}

// F, f at sixteen points per wavefront, everything in registers.  Per point the chain W_2 diag(s) W_1 is 4 HT MFMAs whose
// B operand is s (of THAT point: a DPP row broadcast of the lane that holds it) times W_1 in accumulator layout.
// f = net - F tau needs no reduction either: net - F tau = W_2 (z - s .* (W_1 tau)) + b_2, one more pass of layer 2.
template <int HT, int PP> struct JacPoints {
    static __device__ __forceinline__ void run(const NetRegs<HT> &R, const f32x4 (&w1d)[HT], const f32x4 (&s)[HT], int pass,
                                               long p0, long N, int ns, int n, int q, int r, float *F, const LinLayout &lay)
    {
        if (p0 + PP < N) {
            // all B operands of the point first, then the MFMAs as one block: an MFMA issued right behind the vector
            // instruction that feeds it costs 56 clocks instead of 32 (tools/ubench/mfma16_turn.hip)
            f32x4 g[HT];
#pragma unroll
            for (int to = 0; to < HT; ++to)
#pragma unroll
                for (int v = 0; v < 4; ++v) g[to][v] = bcast<PP>(s[to][v]) * w1d[to][v];
            __builtin_amdgcn_sched_barrier(0);
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
#pragma unroll
            for (int to = 0; to < HT; ++to) {
                a0 = mfma(R.w2[to][0], g[to][0], a0);
                a1 = mfma(R.w2[to][1], g[to][1], a1);
                a2 = mfma(R.w2[to][2], g[to][2], a2);
                a3 = mfma(R.w2[to][3], g[to][3], a3);
            }
            __builtin_amdgcn_sched_barrier(0);
            const f32x4 J = (a0 + a1) + (a2 + a3);
            float *Fb = F + (p0 + PP) * lay.Fp + lay.Fo;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 4 * q + v;
                if (i < ns && r < n) {
                    Fb[i * lay.Fr + r] = J[v] + ((pass && i == r) ? 1.f : 0.f);             // mpc/dynamics.py:118-125
                    if (r < lay.carry) Fb[i * lay.Fr + r - lay.carry] = 0.f;               // (the u_prev columns of this row)
                }
            }
        }
        JacPoints<HT, PP + 1>::run(R, w1d, s, pass, p0, N, ns, n, q, r, F, lay);
    }
};
template <int HT> struct JacPoints<HT, 16> {
    static __device__ __forceinline__ void run(const NetRegs<HT> &, const f32x4 (&)[HT], const f32x4 (&)[HT], int, long, long, int, int,
                                               int, int, float *, const LinLayout &) {}
};

template <int HT, int ACT>
__global__ void __launch_bounds__(64) nn_linearize_fast_kernel(MlpDesc m, long N, int ns, int nc, const float *x, const float *u,
                                                               float *F, float *f, LinLayout lay)
{
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const long p0 = (long)blockIdx.x * 16;
    const long pt = (p0 + r < N) ? p0 + r : N - 1;
    const int n = ns + nc;
    if (lay.carry) write_carry_blocks(lay, p0, N, ns, F, f, lane);       // (first: nothing of the network is in registers yet)
    NetRegs<HT> R;
    load_net<HT>(R, m, q, r);
    f32x4 w1d[HT];                      // W_1 in accumulator layout: rows (hidden units) 16 to + 4q + v, column r
#pragma unroll
    for (int to = 0; to < HT; ++to)
#pragma unroll
        for (int v = 0; v < 4; ++v)
            w1d[to][v] = load_if(m.packed, m.woff[0] + (16 * to + 4 * q + v) * 20 + r, 16 * to < m.wp[1]);
    f32x4 tq;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int fe = 4 * q + v;
        const float tx = load_if(x, pt * lay.xs + lay.xo + fe, fe < ns), tu = load_if(u, pt * nc + (fe - ns), fe >= ns && fe < n);
        tq[v] = fe < ns ? tx : tu;
    }
    f32x4 z[HT], s[HT];
    layer1<HT>(R, tq, z);
#pragma unroll
    for (int to = 0; to < HT; ++to) {
        const f32x4 lin = z[to] - R.b1[to];                     // W_1 tau
        z[to] = act_fn(z[to], ACT);
        s[to] = slope_fn(z[to], ACT);
        z[to] = z[to] - s[to] * lin;
    }
    const f32x4 fv = layer2<HT>(R, z, R.b2);                    // net(x, u) - F [x;u]  (the passthrough x cancels)
    if (p0 + r < N) {
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (4 * q + v < ns) f[pt * lay.fs + lay.fo + 4 * q + v] = fv[v];                 // mpc/mpc.py:508-509
    }
    JacPoints<HT, 0>::run(R, w1d, s, m.pass, p0, N, ns, n, q, r, F, lay);
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


// ---- the host side: ONE layout, ONE validation, ONE plan per entry point, read by the budget query and by the launchers alike
int pad16(int v) { return (v + 15) & ~15; }

// widths -> padded widths, offsets into the packed block, its size (returned in 64 bits: nothing has validated the widths yet)
int64_t mlp_layout(const int *widths, int L, MlpDesc &d)
{
    int64_t off = 0;
    d.L = L;
    for (int l = 0; l <= L; ++l) d.wp[l] = pad16(d.w[l] = widths[l]);
    for (int l = 0; l < L; ++l) {
        d.woff[l] = (int)off; off += (int64_t)d.wp[l + 1] * (d.wp[l] + 4);     // rows padded by 16 bytes (LDS banks), see MlpDesc
        d.boff[l] = (int)off; off += d.wp[l + 1];
    }
    d.total = (int)off;
    return off;
}

int max_hidden_pad(const MlpDesc &d)
{
    int h = 16;
    for (int l = 1; l < d.L; ++l) h = d.wp[l] > h ? d.wp[l] : h;
    return h;
}

// The checks of a description in the order every caller reports them.  NULL, layer count and widths[0] / widths[L] always run,
// the rest by group: a probe by widths alone has no activation, the weight gradient answers a network past the width range
// with its own message, only mlp_prepare has a workspace, a ctrl_carry to honour and pointers to read.
struct MlpCheck { int code; const char *msg; };
enum : unsigned { CK_ACT = 1, CK_RANGE = 2, CK_BIND = 4 };

MlpCheck mlp_check(const mpc_mlp_dynamics *net, int ns, int nc, unsigned what, const void *workspace = nullptr, int64_t bytes = 0)
{
    if (!net) return {MPC_E_NULL, "network is NULL"};
    const int L = net->n_layers;
    if (L < 1 || L > MPC_MLP_MAX_LAYERS) return {MPC_E_ARG, "network: 1..4 Linear layers"};
    if ((what & CK_ACT) && (net->activation < MPC_ACT_SIGMOID || net->activation > MPC_ACT_ELU)) return {MPC_E_ARG, "network: unknown activation"};
    if (net->widths[0] != ns + nc || net->widths[L] != ns) return {MPC_E_DIMS, "network: widths[0] must be n_state + n_ctrl, widths[L] n_state"};
    if ((what & CK_RANGE) && ns > 32) return {MPC_E_DIMS, "network kernels: n_state <= 32"};
    for (int l = 0; l <= L && (what & CK_RANGE); ++l)
        if (net->widths[l] < 1 || net->widths[l] > 4096) return {MPC_E_DIMS, "network: layer width out of range"};
    if (!(what & CK_BIND)) return {MPC_OK, nullptr};
    if (nn_workspace_bytes(net) > bytes || !workspace || ((uintptr_t)workspace & 15))
        return {MPC_E_ARG, "network: workspace too small or not 16-byte aligned (see mpc_mlp_workspace_bytes)"};
    if (net->ctrl_carry != 0 && net->ctrl_carry != nc) return {MPC_E_ARG, "network: ctrl_carry must be 0 or n_ctrl"};
    if (net->ctrl_carry >= ns) return {MPC_E_DIMS, "network: ctrl_carry needs n_state (augmented) > n_ctrl"};
    for (int l = 0; l < L; ++l)
        if (!net->W[l] || !net->b[l]) return {MPC_E_NULL, "network: weight / bias pointer is NULL"};
    return {MPC_OK, nullptr};
}

int refuse(const MlpCheck &c) { set_last_error(c.msg); return c.code; }

// validates the network, lays the packed block out in the workspace and launches the packing kernel
int mlp_prepare(const mpc_mlp_dynamics *net, int ns, int nc, void *workspace, int64_t bytes, MlpDesc &d, hipStream_t st)
{
    const MlpCheck c = mlp_check(net, ns, nc, CK_ACT | CK_RANGE | CK_BIND, workspace, bytes);
    if (c.code) return refuse(c);
    PackArgs a;
    mlp_layout(net->widths, net->n_layers, d);
    d.act = net->activation;
    d.pass = net->passthrough ? 1 : 0;
    d.carry = net->ctrl_carry;
    d.packed = (const float *)workspace;
    for (int l = 0; l < d.L; ++l) a.W[l] = (const float *)net->W[l], a.b[l] = (const float *)net->b[l];
    a.d = d;
    a.dst = (float *)workspace;
    hipLaunchKernelGGL(mlp_pack_kernel, dim3(64), dim3(256), 0, st, a);
    return check_launch("mlp_pack_kernel");
}

// LDS budget of a workgroup: the packed network (when it is staged) + one staging area per wavefront
constexpr size_t LDS_MAX = 160 * 1024, WEIGHTS_IN_LDS_MAX = 96 * 1024;

// What a launch of the rollout / the linearisation does with a network, `groups` of sixteen problems each
struct NnPlan {
    bool fits;                         // false: too wide.  Independent of `groups`: nw shrinks to 1 before a launch is refused
    bool fast, wide, wl;               // the register-resident kernels (no staging) / two state tiles (n_state > 16) / weights in LDS
    int ht;                            // fast: the compile-time hidden-tile bucket, 2, 4, 7 or 8
    int TS, ZS, GT, wave_floats, nw;   // the general kernels: staging strides, floats per wavefront, wavefronts per workgroup
    size_t lds;
    unsigned grid;
};

NnPlan nn_plan(const MlpDesc &d, bool jacobian, bool entry_allows_fast, long groups)
{
    NnPlan pl = {};
    pl.wide = d.w[d.L] > 16;
    // one hidden layer of <= 128 units, n <= 16: the network lives in registers, one wavefront per workgroup
    pl.fast = entry_allows_fast && d.L == 2 && d.wp[0] == 16 && d.wp[1] <= 128;
    if (pl.fast) {
        const int ht = d.wp[1] >> 4;
        pl.ht = ht <= 2 ? 2 : (ht <= 4 ? 4 : (ht <= 7 ? 7 : 8));
        pl.nw = 1;
        pl.grid = (unsigned)groups;
        pl.fits = true;
        return pl;
    }
    const int NTJ = d.wp[0] >> 4;
    pl.TS = d.wp[0] + 4;
    pl.ZS = max_hidden_pad(d) + 4;
    pl.GT = 1;
    for (int l = 1; l < d.L; ++l) pl.GT = (d.wp[l] >> 4) * NTJ > pl.GT ? (d.wp[l] >> 4) * NTJ : pl.GT;
    pl.wave_floats = jacobian ? 16 * pl.TS + (d.L > 1 ? d.L - 1 : 1) * 16 * pl.ZS + 2 * pl.GT * 64 * 4 : 2 * 16 * pl.TS + 2 * 16 * pl.ZS;
    const size_t wbytes = (size_t)d.total * 4, per_wave = (size_t)pl.wave_floats * 4;
    pl.wl = wbytes <= WEIGHTS_IN_LDS_MAX && wbytes + per_wave <= LDS_MAX;
    pl.fits = pl.wl || per_wave <= LDS_MAX;
    // few groups -> one wavefront per workgroup so that every CU gets one
    pl.nw = jacobian && groups >= 4096 ? 8 : (groups >= 2048 ? 4 : (groups >= 1024 ? 2 : 1));
    while (pl.nw > 1 && (pl.wl ? wbytes : 0) + pl.nw * per_wave > LDS_MAX) pl.nw >>= 1;
    pl.lds = (pl.wl ? wbytes : 0) + pl.nw * per_wave;
    pl.grid = (unsigned)((groups + pl.nw - 1) / pl.nw);
    return pl;
}

// rows16: rows readable 16 bytes at a time; the register-resident rollout needs that and n_ctrl <= 4.  A probe that cannot know
// passes false and gets the general kernel's budget, which always holds a network this small (19 KiB a wavefront): the same answer.
NnPlan plan_rollout(const MlpDesc &d, int ns, int nc, bool rows16, long groups) { return nn_plan(d, false, nc <= 4 && rows16, groups); }
NnPlan plan_linearize(const MlpDesc &d, long groups) { return nn_plan(d, true, true, groups); }

const MlpCheck TOO_WIDE = {MPC_E_DIMS, "network: layers too wide for the LDS-resident kernel"};

// runtime value -> template argument: f is a generic lambda and receives a std::integral_constant
template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::integral_constant<bool, V>;
template <typename F> void with_ht(int b, F &&f) { b == 2 ? f(Int<2>{}) : (b == 4 ? f(Int<4>{}) : (b == 7 ? f(Int<7>{}) : f(Int<8>{}))); }
template <typename F> void with_act(int a, F &&f)
{
    a == MPC_ACT_SIGMOID ? f(Int<MPC_ACT_SIGMOID>{}) : (a == MPC_ACT_RELU ? f(Int<MPC_ACT_RELU>{}) : f(Int<MPC_ACT_ELU>{}));
}
template <typename F> void with_bools(bool a, bool b, F &&f)
{
    a ? (b ? f(Bool<true>{}, Bool<true>{}) : f(Bool<true>{}, Bool<false>{})) : (b ? f(Bool<false>{}, Bool<true>{}) : f(Bool<false>{}, Bool<false>{}));
}

// a kernel with dynamic LDS: past 64 KiB the runtime wants to be told
template <typename K, typename... A> void launch_staged(K kernel, unsigned grid, int nw, size_t lds, hipStream_t st, A... args)
{
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * nw), lds, st, args...);
}

#include "nn_param_grad.h"

}  // namespace

// the packed network + slack for alignment; for any description with a legal layer count (nothing else is looked at)
int64_t nn_workspace_bytes(const mpc_mlp_dynamics *net)
{
    if (!net || net->n_layers < 1 || net->n_layers > MPC_MLP_MAX_LAYERS) return 0;
    MlpDesc d;
    return mlp_layout(net->widths, net->n_layers, d) * 4 + 256;
}

// Do the kernels take this network?  The plans the launchers below execute, at one group -- exported as mpc_mlp_supported so
// that a caller can ask BEFORE it routes a module here (a 1024-unit layer is a legal NNDynamics, it keeps the host-driven path).
// bit 0: rollout, bit 1: linearisation, bit 2: its weight gradient (nn_param_grad.h: sigmoid / relu, no ctrl_carry, at most
// PG_MAX_TILES tiles of gW, one point's matrices in LDS) -- answered for a complete description only (W, b non-NULL): a probe
// by widths alone, all that bits 0 and 1 need, keeps its answer.  Silent; d is laid out past validation, pl is valid with bit 2.
static int nn_describe(const mpc_mlp_dynamics *net, int ns, int nc, MlpDesc &d, PgPlan &pl)
{
    if (ns < 1 || nc < 1 || mlp_check(net, ns, nc, CK_RANGE).code) return 0;
    mlp_layout(net->widths, net->n_layers, d);
    bool grad = (net->activation == MPC_ACT_SIGMOID || net->activation == MPC_ACT_RELU) && net->ctrl_carry == 0;
    for (int l = 0; l < d.L; ++l) grad = grad && net->W[l] && net->b[l];
    return (plan_rollout(d, ns, nc, false, 1).fits ? 1 : 0) | (plan_linearize(d, 1).fits ? 2 : 0) | (grad && pg_plan(d, ns, nc, pl) ? 4 : 0);
}

int nn_budget(const mpc_mlp_dynamics *net, int ns, int nc)
{
    MlpDesc d;
    PgPlan pl;
    return nn_describe(net, ns, nc, d, pl);
}

int launch_nn_rollout(const StepParams<float> &p, const mpc_mlp_dynamics *net, void *workspace, int64_t bytes, hipStream_t st)
{
    MlpDesc d;
    int rc = mlp_prepare(net, p.ns, p.nc, workspace, bytes, d, st);
    if (rc) return rc;
    const bool rows16 = (p.ns & 3) == 0 && ((p.ns + p.nc) & 3) == 0 && (!p.C || ((p.C_st & 3) == 0 && (p.C_sb & 3) == 0));
    const NnPlan pl = plan_rollout(d, p.ns, p.nc, rows16, ((long)p.B + 15) / 16);
    if (!pl.fits) return refuse(TOO_WIDE);
    if (pl.fast) {
        with_ht(pl.ht, [&](auto HT) {
            with_act(d.act, [&](auto ACT) {
                constexpr int H = decltype(HT)::value, A = decltype(ACT)::value;
                auto kernel = p.K ? nn_rollout_fast_kernel<H, true, true, A>
                                  : (p.C ? nn_rollout_fast_kernel<H, false, true, A> : nn_rollout_fast_kernel<H, false, false, A>);
                hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(64), 0, st, p, d);
            });
        });
        return check_launch("nn_rollout_fast_kernel");
    }
    with_bools(pl.wl, pl.wide, [&](auto WL, auto WIDE) {
        constexpr bool S = decltype(WL)::value;
        launch_staged(decltype(WIDE)::value ? nn_wide_rollout_kernel<S> : nn_rollout_kernel<S>, pl.grid, pl.nw, pl.lds, st, p, d, pl.TS, pl.ZS,
                      pl.wave_floats);
    });
    return check_launch("nn_rollout_kernel");
}

// both linearisation entries: the same kernels, the layout (dense / the slew-rate augmentation's) a launch parameter
static int launch_linearize(const mpc_mlp_dynamics *net, long N, int ns, int nc, const float *x, const float *u, float *F,
                            float *f, const LinLayout &lay, void *workspace, int64_t bytes, hipStream_t st)
{
    MlpDesc d;
    int rc = mlp_prepare(net, ns, nc, workspace, bytes, d, st);
    if (rc) return rc;
    const NnPlan pl = plan_linearize(d, (N + 15) / 16);
    if (!pl.fits) return refuse(TOO_WIDE);
    if (pl.fast) {
        with_ht(pl.ht, [&](auto HT) {
            with_act(d.act, [&](auto ACT) {
                hipLaunchKernelGGL((nn_linearize_fast_kernel<decltype(HT)::value, decltype(ACT)::value>), dim3(pl.grid), dim3(64), 0, st, d, N,
                                   ns, nc, x, u, F, f, lay);
            });
        });
        return check_launch("nn_linearize_fast_kernel");
    }
    with_bools(pl.wl, pl.wide, [&](auto WL, auto WIDE) {
        constexpr bool S = decltype(WL)::value;
        launch_staged(decltype(WIDE)::value ? nn_wide_linearize_kernel<S> : nn_linearize_kernel<S>, pl.grid, pl.nw, pl.lds, st, d, N, ns, nc,
                      x, u, F, f, lay, pl.TS, pl.ZS, pl.GT, pl.wave_floats);
    });
    return check_launch("nn_linearize_kernel");
}

int launch_nn_linearize(const mpc_mlp_dynamics *net, long N, int ns, int nc, const float *x, const float *u, float *F,
                        float *f, void *workspace, int64_t bytes, hipStream_t st)
{
    if (net && net->ctrl_carry) return refuse({MPC_E_ARG, "mlp_linearize: ctrl_carry describes a rollout only (linearise the network itself)"});
    return launch_linearize(net, N, ns, nc, x, u, F, f, dense_layout(ns, nc), workspace, bytes, st);
}

int launch_nn_linearize_carry(const mpc_mlp_dynamics *net, long N, int ns, int nc, const float *z, const float *u, float *aF,
                              float *af, void *workspace, int64_t bytes, hipStream_t st)
{
    if (net && net->ctrl_carry) return refuse({MPC_E_ARG, "mlp_linearize_carry: pass the network itself (ctrl_carry = 0), not its augmentation"});
    return launch_linearize(net, N, ns, nc, z, u, aF, af, carry_layout(ns, nc), workspace, bytes, st);
}

// workspace of launch_nn_param_grad: the packed network, then one partial per block.  -1: the network is outside the kernel.
int64_t nn_param_grad_workspace_bytes(const mpc_mlp_dynamics *net, int64_t N)
{
    if (!net || net->n_layers < 1 || net->n_layers > MPC_MLP_MAX_LAYERS) return -1;
    const int ns = net->widths[net->n_layers], nc = net->widths[0] - ns;
    MlpDesc d;
    PgPlan pl;
    if (!(nn_describe(net, ns, nc, d, pl) & 4)) return -1;
    return pg_workspace_bytes(pl, N < 0 ? 0 : (long)N);
}

int launch_nn_param_grad(const mpc_mlp_dynamics *net, long N, int ns, int nc, const float *x, const float *u, const float *gF,
                         const float *gf, const mpc_mlp_param_grads *out, void *workspace, int64_t bytes, hipStream_t st)
{
    // this entry's own refusals come before anything else, as MPC_E_DIMS (the module path keeps such a network)
    if (net && net->ctrl_carry) return refuse({MPC_E_DIMS, "mlp_param_grad: ctrl_carry describes a rollout only (differentiate the network itself)"});
    if (net && net->activation == MPC_ACT_ELU) return refuse({MPC_E_DIMS, "mlp_param_grad: sigmoid and relu only (an ELU network keeps the module path)"});
    const MlpCheck c = mlp_check(net, ns, nc, CK_ACT);
    if (c.code) return refuse(c);
    MlpDesc d;
    PgPlan pl;
    if (!(nn_describe(net, ns, nc, d, pl) & 4)) return refuse({MPC_E_DIMS, "mlp_param_grad: the network is outside the kernel (see mpc_mlp_supported, bit 2)"});
    if (bytes < pg_workspace_bytes(pl, N)) return refuse({MPC_E_DIMS, "mlp_param_grad: workspace too small (see mpc_mlp_param_grad_workspace_bytes)"});
    int rc = mlp_prepare(net, ns, nc, workspace, bytes, d, st);
    if (rc) return rc;
    float *partials = reinterpret_cast<float *>(static_cast<char *>(workspace) + pl.packed_bytes);
    const int blocks = pg_blocks(N, pl.nw);
    if (blocks > 0) {
        with_bools(pl.wl, pl.g.ntiles > 16, [&](auto WL, auto MANY) {
            launch_staged(nn_param_grad_kernel<decltype(WL)::value, decltype(MANY)::value ? PG_MAX_TILES : 16>, (unsigned)blocks, pl.nw, pl.lds,
                          st, d, pl.g, N, ns, nc, x, u, gF, gf, partials, pl.TS, pl.ZS, pl.wave_floats);
        });
        rc = check_launch("nn_param_grad_kernel");
        if (rc) return rc;
    }
    PgFinalArgs a = {d.L, pl.g.ntiles, pl.g.psize, blocks};          // (layers past L: zeros and NULL)
    a.partials = partials;
    long entries = 0;
    for (int l = 0; l <= d.L; ++l) { a.w[l] = d.w[l]; a.wp[l] = d.wp[l]; }
    for (int k = 0; k < d.L; ++k) {
        a.tbase[k] = pl.g.tbase[k];
        a.gboff[k] = pl.g.gboff[k];
        a.gW[k] = (float *)out->gW[k];
        a.gb[k] = (float *)out->gb[k];
        entries += (long)d.w[k + 1] * d.w[k] + d.w[k + 1];
    }
    hipLaunchKernelGGL(nn_param_grad_final_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, a);
    return check_launch("nn_param_grad_final_kernel");
}

}  // namespace mpclqr
