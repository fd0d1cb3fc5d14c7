// nn_param_grad64.h -- the backward of the float64 NNDynamics linearisation with respect to the network's weights and biases
// (mpc_mlp_param_grad_dtype with MPC_F64, include/mpc_lqr.h 6d'), on plain float64 FMA.  Included by nn_dynamics64.hip, which
// holds the kernels and the launcher; tests/nn64_grad_host.cpp runs the same statements on the host.
//
// The recursion is the one above mpc_mlp_param_grad in include/mpc_lqr.h (layers l = 1..L, tau = [x;u], a_0 = tau, P_0 = I,
// P_l = diag(s_l) W_l P_{l-1}):
//     G = gF - gf tau',  ch_L = gf,  cM_L = G
//     gW_l += cM_l P_{l-1}' + ch_l a_{l-1}',  gb_l += ch_l,  cP_{l-1} = W_l' cM_l,  ca_{l-1} = W_l' ch_l
//     ch_l = s_l . ca_l + act''(h_l) . rowsum(cP_l . M_l),  cM_l = diag(s_l) cP_l          (l < L)
// Sigmoid and relu.  Sigmoid: act'' . rowsum(cP . M) = (1 - 2a) . rowsum(cP . P) -- no M is kept, nothing is divided by a slope;
// relu: that term is 0.
//
// A BLOCK of PG64_THREADS threads works on one point at a time.  Written as nn_dynamics64.h is, against an executor that answers
// lane() / xor_get() for the thread's wavefront, and for the block
//     ex.tid()        this thread, 0 .. PG64_THREADS - 1 (its wavefront is tid() >> 6)
//     ex.sync()       the block's barrier: LDS stores so far are visible to every thread's loads from here on
// The wavefronts split each product of the chain.  Every returned entry of gW / gb -- entry e of the list [gW_1, gb_1, ..., gW_L,
// gb_L], each in nn.Linear's row-major layout -- is owned by exactly one thread: e = tid + k * PG64_THREADS, k < KMAX, with KMAX
// a template constant and the loop over k unrolled under a predicate, so that the sums sit in fixed registers across the block's
// grid-stride loop over its points.  A block then writes its KMAX * PG64_THREADS sums as one partial into the workspace (entry e
// at offset e) and a second launch adds the partials in block order: no atomics, every sum in a fixed order, bitwise
// reproducible, and nothing depends on what outputs or workspace held before.
//
// LDS of a block (doubles; rows of every [.. x n] matrix on the odd stride n | 1): tau [n], the hidden activations a_1 .. a_{L-1},
// two vectors for ch / ca, two ping-pong buffers for cM / cP, and P_2 .. P_{L-1}.  P_1 = diag(s_1) W_1 is never stored: it is
// read as s_1[i] * W_1[i][j] where the weights are (the staged copy, or nn.Linear's tensor when the network is read in place).
// Each product has one call site per address space of its operands, so no LDS operand is read through a generic pointer.
#pragma once
#include "nn_dynamics64.h"

// the grid: min(N, this) blocks, one point per block and pass
#define MPC_MLP_PARAM_GRAD64_MAX_BLOCKS 512

namespace mpclqr {
namespace nn64 {

constexpr int PG64_THREADS = 512;
// the instantiations of KMAX: a network with at most KMAX * PG64_THREADS weights and biases takes the smallest that holds it
constexpr int PG64_KMAX_SMALL = 8, PG64_KMAX_MID = 16, PG64_KMAX_LARGE = 40;

struct GradLayout {
    int ldn;                 // row stride of the [.. x n] matrices
    int rmax;                // doubles of one ch vector = max(w[1] .. w[L])
    int szA, szB;            // the ping-pong buffers: cM_L, cM_{L-2}, ... live in A, cM_{L-1}, ... in B
    int pst;                 // P_2 .. P_{L-1}
    long entries;            // weights and biases in all
    long doubles;            // the block's area
};

inline GradLayout grad_layout(const Net &m)
{
    GradLayout g = {};
    const int L = m.L;
    g.ldn = m.w[0] | 1;
    long szA = 0, szB = 0, pst = 0;
    for (int l = 1; l <= L; ++l) {
        const long sz = (long)m.w[l] * g.ldn;
        if (m.w[l] > g.rmax) g.rmax = m.w[l];
        if ((L - l) & 1) szB = sz > szB ? sz : szB;
        else szA = sz > szA ? sz : szA;
        if (l >= 2 && l <= L - 1) pst += sz;
        g.entries += (long)m.w[l] * m.w[l - 1] + m.w[l];
    }
    g.doubles = (long)m.w[0] + m.zsum + 2L * g.rmax + szA + szB + pst;
    // (a caller that launches has checked `doubles` against the LDS of a workgroup: the three sizes then fit an int)
    g.szA = (int)szA; g.szB = (int)szB; g.pst = (int)pst;
    return g;
}

// the smallest KMAX instantiation that owns `entries` weights and biases, 0: none does
inline int grad_kmax(long entries)
{
    if (entries <= (long)PG64_KMAX_SMALL * PG64_THREADS) return PG64_KMAX_SMALL;
    if (entries <= (long)PG64_KMAX_MID * PG64_THREADS) return PG64_KMAX_MID;
    if (entries <= (long)PG64_KMAX_LARGE * PG64_THREADS) return PG64_KMAX_LARGE;
    return 0;
}

// sum_k a[k * as] b[k * bs], two chains
NN64_FN double dot_strided(const double *a, int as, const double *b, int bs, int n)
{
    double s0 = 0.0, s1 = 0.0;
    int k = 0;
    for (; k + 1 < n; k += 2) {
        s0 = fma(a[k * as], b[k * bs], s0);
        s1 = fma(a[(k + 1) * as], b[(k + 1) * bs], s1);
    }
    if (k < n) s0 = fma(a[k * as], b[k * bs], s0);
    return s0 + s1;
}

// sum_k w[k] slope(a[k]) b[k * bs]: a row of W_2 against a column of P_1 = diag(s_1) W_1
NN64_FN double dot_sloped(const double *w, const double *a, int act, const double *b, int bs, int n)
{
    double s0 = 0.0, s1 = 0.0;
    int k = 0;
    for (; k + 1 < n; k += 2) {
        s0 = fma(w[k] * slope_fn(a[k], act), b[k * bs], s0);
        s1 = fma(w[k + 1] * slope_fn(a[k + 1], act), b[(k + 1) * bs], s1);
    }
    if (k < n) s0 = fma(w[k] * slope_fn(a[k], act), b[k * bs], s0);
    return s0 + s1;
}

// ---------------------------------------------------------------------------------------------------------------
// One point's contribution to the block's sums.  area: grad_layout(m).doubles doubles of the block's own; acc: this thread's
// KMAX sums, entry tid + k * PG64_THREADS in acc[k].  Every thread of the block calls it.
// ---------------------------------------------------------------------------------------------------------------
template <bool WL, int KMAX, class X>
NN64_FN void param_grad_point(X &ex, const Net &m, const GradLayout &g, const double *staged, double *area, const double *x, const double *u,
                              const double *gF, const double *gf, double (&acc)[KMAX])
{
    const int tid = ex.tid(), nt = PG64_THREADS, wave = tid >> 6, nw = PG64_THREADS >> 6;
    const int L = m.L, n = m.w[0], ns = m.w[L], ldn = g.ldn, act = m.act;
    double *tau = area, *as = tau + n, *chA = as + m.zsum, *chB = chA + g.rmax, *bufA = chB + g.rmax, *bufB = bufA + g.szA, *pst = bufB + g.szB;
    const double *W1 = weights_of<WL>(m, staged, 0);
    const int ld1 = stride_of<WL>(m, 0);

    for (int i = tid; i < n; i += nt) tau[i] = i < ns ? x[i] : u[i - ns];
    ex.sync();
    // the hidden activations a_1 .. a_{L-1}: each wavefront takes a run of a layer's outputs (the network's output is not needed)
    {
        const double *in = tau;
        double *out = as;
        for (int l = 0; l + 1 < L; ++l) {
            const int wo = m.w[l + 1], per = (wo + nw - 1) / nw, o0 = wave * per, cnt = wo - o0 < per ? wo - o0 : per;
            const int ld = stride_of<WL>(m, l);
            if (cnt > 0)
                layer(ex, weights_of<WL>(m, staged, l) + (long)o0 * ld, ld, bias_of<WL>(m, staged, l) + o0, in, m.w[l], out + o0, cnt, true, act);
            ex.sync();
            in = out;
            out += wo;
        }
    }
    // P_l = diag(s_l) W_l P_{l-1} for l = 2 .. L-1, one entry a thread and turn.  The first product reads P_1 where the weights
    // are, every later one an LDS matrix: two call sites
    {
        double *dst = pst;
        const double *ap = as;                                   // a_{l-1}
        for (int l = 2; l <= L - 1; ++l) {
            const int wi = m.w[l - 1], wo = m.w[l];
            const double *Wl = weights_of<WL>(m, staged, l - 1), *al = ap + wi;
            const int ld = stride_of<WL>(m, l - 1);
            if (l == 2) {
                for (int e = tid; e < wo * n; e += nt) {
                    const int i = e / n, j = e - i * n;
                    dst[i * ldn + j] = slope_fn(al[i], act) * dot_sloped(Wl + (long)i * ld, ap, act, W1 + j, ld1, wi);
                }
            } else {
                const double *src = dst - wi * ldn;
                for (int e = tid; e < wo * n; e += nt) {
                    const int i = e / n, j = e - i * n;
                    dst[i * ldn + j] = slope_fn(al[i], act) * dot_strided(Wl + (long)i * ld, 1, src + j, ldn, wi);
                }
            }
            ex.sync();
            dst += wo * ldn;
            ap = al;
        }
    }
    // cM_L = G = gF - gf tau', ch_L = gf
    for (int e = tid; e < ns * n; e += nt) {
        const int i = e / n, j = e - i * n;
        bufA[i * ldn + j] = fma(-gf[i], tau[j], gF[e]);
    }
    for (int i = tid; i < ns; i += nt) chA[i] = gf[i];
    ex.sync();

    double *cM = bufA, *cN = bufB, *ch = chA, *cn = chB;
    int ebase = (int)g.entries;                                  // layer l's entries are [ebase, ebase + wo * wi + wo)
    const double *ap = as + m.zsum;                              // a_{l-1}, walked down
    const double *Pp = pst + g.pst;                              // P_{l-1} for l - 1 >= 2, walked down
    for (int l = L; l >= 1; --l) {
        const int wo = m.w[l], wi = m.w[l - 1], nW = wo * wi;
        ebase -= nW + wo;
        if (l >= 2) ap -= wi;
        if (l >= 3) Pp -= wi * ldn;
        // this thread's entries of gW_l and gb_l
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const int r = tid + k * nt - ebase;
            if (r >= 0 && r < nW + wo) {
                double v;
                if (r >= nW) {
                    v = ch[r - nW];
                } else {
                    const int i = r / wi, j = r - i * wi;
                    if (l == 1) v = fma(ch[i], tau[j], cM[i * ldn + j]);                               // P_0 = I
                    else if (l == 2) v = fma(ch[i], ap[j], slope_fn(ap[j], act) * dot_part(cM + i * ldn, W1 + (long)j * ld1, n, 0, 1));
                    else v = fma(ch[i], ap[j], dot_part(cM + i * ldn, Pp + j * ldn, n, 0, 1));
                }
                acc[k] += v;
            }
        }
        if (l == 1) break;
        // cP_{l-1} = W_l' cM_l into the other buffer, ca_{l-1} = W_l' ch_l into the other vector
        const double *Wl = weights_of<WL>(m, staged, l - 1);
        const int ld = stride_of<WL>(m, l - 1);
        for (int e = tid; e < wi * n; e += nt) {
            const int i = e / n, j = e - i * n;
            cN[i * ldn + j] = dot_strided(Wl + i, ld, cM + j, ldn, wo);
        }
        for (int i = tid; i < wi; i += nt) cn[i] = dot_strided(Wl + i, ld, ch, 1, wo);
        ex.sync();
        // row i of it: ch_{l-1}[i] = s ca + (1 - 2a) rowsum(cP . P_{l-1}), then cM_{l-1} = s cP in place
        for (int i = tid; i < wi; i += nt) {
            const double a = ap[i], s = slope_fn(a, act);
            double *row = cN + i * ldn;
            double rs = 0.0;
            if (act == MPC_ACT_SIGMOID) {
                if (l == 2) rs = s * dot_part(row, W1 + (long)i * ld1, n, 0, 1);
                else rs = dot_part(row, Pp + i * ldn, n, 0, 1);
            }
            cn[i] = fma(s, cn[i], (1.0 - 2.0 * a) * rs);
            for (int j = 0; j < n; ++j) row[j] *= s;
        }
        ex.sync();
        double *t = cM; cM = cN; cN = t;
        t = ch; ch = cn; cn = t;
    }
    ex.sync();      // (the block's next point overwrites the area)
}

// The second launch's work for entry e: the partials in block order, stored where nn.Linear keeps that weight or bias
struct GradFinal {
    int L, blocks;
    long stride;                                   // doubles from one block's partial to the next = KMAX * PG64_THREADS
    int w[MPC_MLP_MAX_LAYERS + 1];
    const double *partials;
    double *gW[MPC_MLP_MAX_LAYERS], *gb[MPC_MLP_MAX_LAYERS];
};

NN64_FN void sum_partials(const GradFinal &a, long e)
{
    double s = 0.0;
    for (int b = 0; b < a.blocks; ++b) s += a.partials[b * a.stride + e];
    long base = 0;
#pragma unroll
    for (int l = 0; l < MPC_MLP_MAX_LAYERS; ++l) {
        if (l < a.L) {
            const long nW = (long)a.w[l + 1] * a.w[l], r = e - base;
            if (r >= 0 && r < nW) a.gW[l][r] = s;
            else if (r >= nW && r < nW + a.w[l + 1]) a.gb[l][r - nW] = s;
            base += nW + a.w[l + 1];
        }
    }
}

}  // namespace nn64
}  // namespace mpclqr
