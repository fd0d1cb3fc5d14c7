// nn_dynamics64.h -- mpc.dynamics.NNDynamics in float64 on plain FMA: the per-problem rollout / line search and the per-point
// linearisation that nn_dynamics64.hip launches with one wavefront per problem (point).
//
// Plain C++ written once for sixty-four lanes that run in step: every function takes an executor `X` that answers
//     ex.lane()              this lane, 0..63
//     ex.sync()              the lanes' LDS stores so far are visible to the lanes' LDS loads from here on
//     ex.xor_get(v, mask)    lane (lane ^ mask)'s v; every lane of the wavefront calls it
// The kernels pass the wavefront itself (nn_dynamics64.hip: WaveExec -- a compiler fence, __shfl_xor); a host build passes
// sixty-four threads around a barrier and runs the same statements (tests/nn64_host.cpp), which is how the arithmetic is checked in
// float64 without a GPU and where a host sanitizer sees it.
//
// Work split of every matrix-vector product: S lanes per output (S the largest power of two with S * outputs <= 64), lane (o, s)
// sums the terms j = s, s + S, ... in four interleaved chains, the S partials meet in an xor butterfly -- a fixed order: the
// results are bitwise reproducible.  No atomics, no approximate exp / reciprocal: exp, expm1 and a real division.
#pragma once
#include <math.h>
#include "lqr_params.h"

#if defined(__HIPCC__)
#define NN64_FN __host__ __device__ __forceinline__
#else
#define NN64_FN inline
#endif

namespace mpclqr {
namespace nn64 {

// The network as a kernel reads it.  W[l] / b[l]: nn.Linear's own tensors (row-major [w[l+1]][w[l]]).  A block that stages the
// network copies it into LDS first: W_l at soff[l] with rows of ld[l] = w[l] | 1 doubles (an odd stride: the rows S = 1 lanes
// read side by side fall on different banks), b_l at sboff[l]; `total` doubles in all.  The kernels read this struct from an LDS
// copy: it is indexed by the layer at run time, which a kernel argument cannot be without a trip through scratch.
struct Net {
    int L, act, pass, carry;
    int w[MPC_MLP_MAX_LAYERS + 1];
    int ld[MPC_MLP_MAX_LAYERS], soff[MPC_MLP_MAX_LAYERS], sboff[MPC_MLP_MAX_LAYERS];
    int total;
    int zmax;                    // rollout: doubles of one activation buffer = max(hidden widths, n_state)
    int zsum, gmax;              // linearisation: sum of the hidden widths; columns of a chain buffer = max(w[0] .. w[L-2])
    const double *W[MPC_MLP_MAX_LAYERS], *b[MPC_MLP_MAX_LAYERS];
};

inline void net_layout(Net &m)
{
    int off = 0, zmax = m.w[m.L], zsum = 0, gmax = m.w[0];
    for (int l = 0; l < m.L; ++l) {
        m.ld[l] = m.w[l] | 1;
        m.soff[l] = off; off += m.w[l + 1] * m.ld[l];
        m.sboff[l] = off; off += m.w[l + 1];
        if (l >= 1) { zmax = m.w[l] > zmax ? m.w[l] : zmax; zsum += m.w[l]; }
        if (l >= 1 && l <= m.L - 2) gmax = m.w[l] > gmax ? m.w[l] : gmax;
    }
    m.total = off; m.zmax = zmax; m.zsum = zsum; m.gmax = gmax;
}
// doubles of LDS one wavefront works in
inline long rollout_wave_doubles(const Net &m) { return 2L * m.w[0] + 2L * m.zmax; }
inline long linearize_wave_doubles(const Net &m)
{
    return (long)m.w[0] + m.zsum + m.w[m.L] + (long)m.w[m.L] * m.gmax * (m.L >= 3 ? 2 : 1);
}

// where layer l's weights / biases are read: the staged copy (WL) or the tensors themselves through the caches
template <bool WL> NN64_FN const double *weights_of(const Net &m, const double *staged, int l) { return WL ? staged + m.soff[l] : m.W[l]; }
template <bool WL> NN64_FN const double *bias_of(const Net &m, const double *staged, int l) { return WL ? staged + m.sboff[l] : m.b[l]; }
template <bool WL> NN64_FN int stride_of(const Net &m, int l) { return WL ? m.ld[l] : m.w[l]; }

// a block's threads copy the network into LDS (the caller synchronises the block afterwards)
NN64_FN void stage_net(const Net &m, double *staged, int tid, int nthreads)
{
    for (int l = 0; l < m.L; ++l) {
        const int in = m.w[l], out = m.w[l + 1], ld = m.ld[l];
        for (int e = tid; e < out * ld; e += nthreads) {
            const int o = e / ld, j = e - o * ld;
            staged[m.soff[l] + e] = j < in ? m.W[l][(long)o * in + j] : 0.0;
        }
        for (int o = tid; o < out; o += nthreads) staged[m.sboff[l] + o] = m.b[l][o];
    }
}

// log2 of S, the lanes per output
NN64_FN int split_log2(int outputs)
{
    int k = 0;
    while ((2 << k) * outputs <= 64) ++k;
    return k;
}

// terms j = s, s + S, ... of sum_j w[j] a[j], four chains
NN64_FN double dot_part(const double *w, const double *a, int n, int s, int S)
{
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = s;
    for (; j + 3 * S < n; j += 4 * S) {
        a0 = fma(w[j], a[j], a0);
        a1 = fma(w[j + S], a[j + S], a1);
        a2 = fma(w[j + 2 * S], a[j + 2 * S], a2);
        a3 = fma(w[j + 3 * S], a[j + 3 * S], a3);
    }
    for (; j < n; j += S) a0 = fma(w[j], a[j], a0);
    return (a0 + a1) + (a2 + a3);
}

// the sum over the S adjacent lanes of a group (S a power of two), in every lane of it
template <class X> NN64_FN double group_sum(X &ex, double v, int S)
{
    for (int m = 1; m < S; m <<= 1) v += ex.xor_get(v, m);
    return v;
}

NN64_FN double act_fn(double a, int kind)
{
    if (kind == MPC_ACT_SIGMOID) return 1.0 / (1.0 + exp(-a));
    if (kind == MPC_ACT_RELU) return a > 0.0 ? a : 0.0;
    return a > 0.0 ? a : expm1(a);                                    // F.elu, alpha = 1
}
// derivative of the activation from its OUTPUT (mpc/dynamics.py:104-112)
NN64_FN double slope_fn(double z, int kind)
{
    if (kind == MPC_ACT_SIGMOID) return z * (1.0 - z);
    if (kind == MPC_ACT_RELU) return z > 0.0 ? 1.0 : 0.0;
    return z > 0.0 ? 1.0 : z + 1.0;
}

// out[o] = act(sum_j W[o][j] in[j] + b[o]) for the `wo` outputs of one layer (no activation when !hidden); in / out in LDS.
// The caller synchronises before `out` is read.
template <class X>
NN64_FN void layer(X &ex, const double *W, int ld, const double *bias, const double *in, int wi, double *out, int wo, bool hidden, int act)
{
    const int k = split_log2(wo), S = 1 << k, lane = ex.lane(), s = lane & (S - 1);
    for (int base = 0; base < wo; base += 64 >> k) {
        const int o = base + (lane >> k);
        const bool ok = o < wo;
        const double part = ok ? dot_part(W + (long)o * ld, in, wi, s, S) : 0.0;
        const double v = group_sum(ex, part, S) + (ok ? bias[o] : 0.0);
        if (ok && s == 0) out[o] = hidden ? act_fn(v, act) : v;
    }
}

// One row's share of J_t(tau') - J_t(tau_nominal) for the stage cost 0.5 tau'C tau + c'tau, any C (csrc/nn_dynamics.hip,
// line_search_delta): 0.5 [ d'(C tau') + tb'(C d) ] + c'd with d = tau' - tb, from s = (C tau')_i and s2 = (C d)_i
NN64_FN double line_search_delta(double tau_i, double d_i, double s, double s2, double c_i)
{
    return fma(d_i, fma(0.5, s, c_i), 0.5 * (tau_i - d_i) * s2);
}

// ---------------------------------------------------------------------------------------------------------------
// lqr_forward through the network (mpc/lqr_step.py:164-261) for problem b -- the semantics of nn_rollout_kernel
// (csrc/nn_dynamics.hip), include/mpc_lqr.h (6d).  area: rollout_wave_doubles(m) doubles of this wavefront's own.
// ---------------------------------------------------------------------------------------------------------------
template <bool WL, class X>
NN64_FN void rollout_problem(X &ex, const StepParams<double> &p, const Net &m, const double *staged, double *area, long b)
{
    const int lane = ex.lane();
    const int ns = p.ns, nc = p.nc, n = ns + nc, T = p.T;
    const long B = p.B;
    double *tau = area, *dd = tau + n, *z0 = dd + n, *z1 = z0 + m.zmax;
    const bool has_gain = p.K != nullptr, has_cost = p.C != nullptr;
    const double old_cost = p.old_costs_in ? p.old_costs_in[b] : 0.0;
    const int kc = split_log2(nc), Sc = 1 << kc, kn = split_log2(n), Sn = 1 << kn;
    double alpha = 1.0, cost = 0.0, dun = 0.0, full = 0.0;
    const int max_ls = has_gain ? p.max_ls : 1;
    for (int pass = 0; pass < max_ls; ++pass) {
        for (int i = lane; i < n; i += 64) {
            const double x = i < ns ? p.x_init[b * ns + i] : 0.0;
            tau[i] = x;
            dd[i] = (has_gain && i < ns) ? x - p.cur_x[b * ns + i] : 0.0;                    // :227
            if (i < ns) p.new_x[b * ns + i] = x;
        }
        ex.sync();
        double ca = 0.0, da = 0.0;
        for (int t = 0; t < T; ++t) {
            const long tb = (long)t * B + b;
            for (int base = 0; base < nc; base += 64 >> kc) {
                const int i = base + (lane >> kc), s = lane & (Sc - 1);
                const bool ok = i < nc;
                double g = 0.0;
                if (has_gain) {
                    // (dx_0 = 0 whatever current_x[0] is, :182; dd keeps tau' - tau_nominal for the cost difference below)
                    g = (ok && t > 0) ? dot_part(p.K + (tb * nc + i) * ns, dd, ns, s, Sc) : 0.0;
                    g = group_sum(ex, g, Sc);
                }
                if (ok && s == 0) {
                    const double u = p.cur_u[tb * nc + i];
                    double un = u;
                    if (has_gain) {
                        un = g + u + alpha * p.k[tb * nc + i];                              // :192
                        if (p.zero_mask && p.zero_mask[tb * nc + i]) un = 0.0;              // :197-198
                        if (p.bound_mode != MPC_BOUND_NONE) {                               // :200-213
                            double lo = p.bound_mode == MPC_BOUND_SCALAR ? p.lo_s : p.lo[tb * nc + i];
                            double hi = p.bound_mode == MPC_BOUND_SCALAR ? p.hi_s : p.hi[tb * nc + i];
                            if (p.has_delta) {
                                const double l2 = u - p.delta_u, h2 = u + p.delta_u;
                                lo = (l2 < lo) ? lo : l2;
                                hi = (h2 > hi) ? hi : h2;
                            }
                            if (un < lo) un = lo;                                           // util.eclamp
                            if (un > hi) un = hi;
                        }
                        p.new_u[tb * nc + i] = un;
                    }
                    tau[ns + i] = un;
                    const double d = u - un;
                    dd[ns + i] = -d;
                    da = fma(d, d, da);
                }
            }
            ex.sync();
            if (has_cost) {                                                                 // :230-232
                const double *Ct = p.C + (long)t * p.C_st + b * p.C_sb;
                const double *ct = p.c + (long)t * p.c_st + b * p.c_sb;
                for (int base = 0; base < n; base += 64 >> kn) {
                    const int i = base + (lane >> kn), s = lane & (Sn - 1);
                    const bool ok = i < n;
                    double r1 = ok ? dot_part(Ct + (long)i * n, tau, n, s, Sn) : 0.0;
                    double r2 = (ok && has_gain) ? dot_part(Ct + (long)i * n, dd, n, s, Sn) : 0.0;
                    r1 = group_sum(ex, r1, Sn);
                    if (has_gain) r2 = group_sum(ex, r2, Sn);
                    if (ok && s == 0) {
                        // with gains the line search's J(tau') - J(nominal) (:176-179), summed as a difference
                        if (has_gain) ca += line_search_delta(tau[i], dd[i], r1, r2, ct[i]);
                        else ca = fma(tau[i], fma(0.5, r1, ct[i]), ca);
                    }
                }
            }
            if (t < T - 1) {                                                                // :223-225
                const double *in = tau;
                double *out = z0;
                for (int l = 0; l < m.L; ++l) {
                    layer(ex, weights_of<WL>(m, staged, l), stride_of<WL>(m, l), bias_of<WL>(m, staged, l), in, m.w[l], out, m.w[l + 1],
                          l + 1 < m.L, m.act);
                    ex.sync();
                    in = out;
                    out = out == z0 ? z1 : z0;
                }
                for (int i = lane; i < ns; i += 64) {
                    // mpc/dynamics.py:74-75; an augmented state's first entries are the control just applied (:139-147)
                    const double skip = i < m.carry ? tau[ns + i] : (m.pass ? tau[i] : 0.0);
                    const double xn = in[i] + skip;
                    const long at = ((long)(t + 1) * B + b) * ns + i;
                    tau[i] = xn;
                    dd[i] = has_gain ? xn - p.cur_x[at] : 0.0;
                    p.new_x[at] = xn;
                }
                ex.sync();
            }
        }
        ca = group_sum(ex, ca, 64);
        da = group_sum(ex, da, 64);
        const double dn = sqrt(da);
        if (pass == 0) full = dn;                                                           // :243-245
        cost = has_gain ? old_cost + ca : ca;
        dun = dn;
        // :176-179, 247: keep shrinking while this problem's cost got worse; the last trial is kept
        if (!(has_gain && ca > 0.0 && pass + 1 < max_ls)) break;
        alpha *= p.ls_decay;
    }
    if (lane == 0) {
        if (p.costs) p.costs[b] = cost;
        if (p.old_costs) p.old_costs[b] = old_cost;
        if (p.full_du_norm) p.full_du_norm[b] = full;
        if (p.alpha_du_norm) p.alpha_du_norm[b] = dun;
        if (p.alphas) p.alphas[b] = alpha;
        if (p.status && (!(fabs(cost) <= 1.7976931348623157e308))) p.status[b] |= MPC_ST_NONFINITE;
    }
}

// One product of the linearisation's chain: dst [rows, wj] = (G [rows, wh] diag(sl)) W [wh, wj]; lane e, e + 64, ... owns entries of dst
NN64_FN void chain_product(int lane, const double *G, int gld, const double *sl, const double *W, int wld, double *dst, int rows, int wh, int wj)
{
    for (int e = lane; e < rows * wj; e += 64) {
        const int i = e / wj, j = e - i * wj;
        const double *Gi = G + (long)i * gld;
        double a0 = 0.0, a1 = 0.0;
        int h = 0;
        for (; h + 1 < wh; h += 2) {
            a0 = fma(Gi[h] * sl[h], W[(long)h * wld + j], a0);
            a1 = fma(Gi[h + 1] * sl[h + 1], W[(long)(h + 1) * wld + j], a1);
        }
        if (h < wh) a0 = fma(Gi[h] * sl[h], W[(long)h * wld + j], a0);
        dst[e] = a0 + a1;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// MPC.linearize_dynamics(ANALYTIC) at one point (mpc/mpc.py:495-512, NNDynamics.grad_input mpc/dynamics.py:82-128):
// F [ns, n] = W_L diag(s_{L-1}) W_{L-1} ... diag(s_1) W_1 (+ I on the state block), f = net(x, u) - F [x;u].  The chain is
// accumulated from the OUTPUT side, G_l = (G_{l+1} diag(s_l)) W_l with G_L = W_L: every intermediate has n_state rows.
// area: linearize_wave_doubles(m) doubles of this wavefront's own.
// ---------------------------------------------------------------------------------------------------------------
template <bool WL, class X>
NN64_FN void linearize_point(X &ex, const Net &m, const double *staged, double *area, int ns, int nc, const double *x, const double *u,
                             double *F, double *f)
{
    const int lane = ex.lane(), n = ns + nc, L = m.L;
    double *tau = area, *zs = tau + n, *o = zs + m.zsum, *ga = o + ns, *gb = ga + (long)ns * m.gmax;
    for (int i = lane; i < n; i += 64) tau[i] = i < ns ? x[i] : u[i - ns];
    ex.sync();
    {
        const double *in = tau;
        double *out = zs;
        for (int l = 0; l < L; ++l) {
            double *dst = l + 1 < L ? out : o;
            layer(ex, weights_of<WL>(m, staged, l), stride_of<WL>(m, l), bias_of<WL>(m, staged, l), in, m.w[l], dst, m.w[l + 1], l + 1 < L, m.act);
            ex.sync();
            in = dst;
            out += m.w[l + 1];
        }
    }
    // activations -> slopes (in place), the output -> net(x, u)
    for (int i = lane; i < m.zsum; i += 64) zs[i] = slope_fn(zs[i], m.act);
    if (m.pass)
        for (int i = lane; i < ns; i += 64) o[i] += tau[i];
    ex.sync();
    // the chain; the last product (l = 1) lands in ga.  The first product reads G_L = W_L where the weights are (global memory when the
    // network is not staged), every later one an LDS buffer: two call sites, so that each keeps the address space of its operand and
    // no load of LDS data is a generic one
    double *dst = ((L - 1) & 1) ? ga : gb;                 // L - 1 products, alternating, the last one into ga
    const double *sl = zs + m.zsum;
    if (L == 1) {
        const double *W1 = weights_of<WL>(m, staged, 0);
        const int ld1 = stride_of<WL>(m, 0);
        for (int e = lane; e < ns * n; e += 64) ga[e] = W1[(long)(e / n) * ld1 + (e % n)];
    } else {
        sl -= m.w[L - 1];
        chain_product(lane, weights_of<WL>(m, staged, L - 1), stride_of<WL>(m, L - 1), sl, weights_of<WL>(m, staged, L - 2),
                      stride_of<WL>(m, L - 2), dst, ns, m.w[L - 1], m.w[L - 2]);
        ex.sync();
    }
    for (int l = L - 2; l >= 1; --l) {
        double *src = dst;
        dst = dst == ga ? gb : ga;
        sl -= m.w[l];
        chain_product(lane, src, m.w[l], sl, weights_of<WL>(m, staged, l - 1), stride_of<WL>(m, l - 1), dst, ns, m.w[l], m.w[l - 1]);
        ex.sync();
    }
    if (L == 1) ex.sync();
    if (m.pass)
        for (int i = lane; i < ns; i += 64) ga[i * n + i] += 1.0;
    ex.sync();
    for (int e = lane; e < ns * n; e += 64) F[e] = ga[e];
    {
        const int k = split_log2(ns), S = 1 << k, s = lane & (S - 1);
        for (int base = 0; base < ns; base += 64 >> k) {
            const int i = base + (lane >> k);
            const bool ok = i < ns;
            const double part = ok ? dot_part(ga + (long)i * n, tau, n, s, S) : 0.0;
            const double r = group_sum(ex, part, S);
            if (ok && s == 0) f[i] = o[i] - r;
        }
    }
    ex.sync();      // (the next point of this wavefront's loop overwrites the area)
}

}  // namespace nn64
}  // namespace mpclqr
