// nn_param_grad.h -- the other half of nn_linearize_kernel: the gradient of a loss with respect to the network's weights
// and biases, given the cotangents gF [N, ns, n] and gf [N, ns] of F = d net / d [x;u] and f = net(x, u) - F [x;u]
// (x, u constants).  Included at the end of nn_dynamics.hip, inside its namespaces (it uses MlpDesc, mlp_forward,
// stage_weights, mlp_prepare).  fp32, sixteen points per wavefront like every kernel of that file.
//
// Layers k = 0 .. L-1, W_k [w_{k+1} x w_k], a_0 = tau, a_k = sigma(W_{k-1} a_{k-1} + b_{k-1}), slopes s_k, and the chain
// P_0 = I_n, P_k = diag(s_k) W_{k-1} P_{k-1}  [w_k x n].  Every matrix of a point carries ONE MORE COLUMN, column n:
//
//     Pt_k = [ P_k | a_k ]            (Pt_0 = [ I | tau ])
//     Ct_L = [ gF - gf tau' | gf ]    the cotangent of (W_{L-1} P_{L-1}, W_{L-1} a_{L-1} + b_{L-1})
//     Ct_k = [ s_k . cP_k | s_k . ca_k + sigma''(h_k) . rowsum(cP_k . M_k) ],   [ cP_k | ca_k ] = W_k' Ct_{k+1}
//
// so that the vector chain (ca, ch of the issue's recursion) rides in the same MFMAs as the matrix chain, and
//
//     gW_k = sum over points of Ct_{k+1} Pt_k'          gb_k = sum over points of column n of Ct_{k+1}.
//
// sigma''(h) . rowsum(cP . M) needs no M: for the sigmoid sigma'' = s (1 - 2z), and s . M = P, so it is
// (1 - 2z) . rowsum(cP . P) over the columns j < n; for relu it is 0.  (ELU is refused by the launcher.)
//
// Padding: widths are padded to 16 by zero rows / columns of the packed weights.  A padded hidden row has h = 0 (a = 0.5,
// s = 0.25 for the sigmoid): its row of P_k is s . 0 = 0, its entry of column n is written as 0 explicitly, its row of
// [cP_k | ca_k] is 0 because the column of W_k it is multiplied with is 0.  Padded tile entries are never written out.
//
// LDS per wavefront: tau and the activations of its sixteen points (as in nn_linearize_kernel), then for ONE point at a
// time Pt_0 .. Pt_{L-1} and Ct_1 .. Ct_L, row-major with row stride JS = NC + 4 (NC = n + 1 rounded up to 16), then gb.
// The gW tiles (16 x 16, accumulator layout) stay in registers across the wavefront's grid-stride loop over groups of
// sixteen points; the tile list is a kernel argument so that tile t is register quadruple t (a compile-time index).
// At the end the block's wavefronts are added in wave order through LDS and the block writes ONE partial; a second
// launch adds the partials in block order.  No atomics; nothing is read that the same call did not write.

constexpr int PG_MAX_TILES = 40;       // 16 x 16 tiles of all gW_k together (32/8 with one hidden layer of 100: 35)
constexpr int PG_MAX_BLOCKS = 256;     // one workgroup per CU
constexpr int PG_MAX_WAVES = 4;        // one wavefront per SIMD

struct PgDesc {
    int NC, JS;                        // columns of a point's matrices (n + 1 padded to 16), row stride
    int ntiles, gbtotal, psize;        // tiles, bias slots (sum of padded widths), floats of one partial
    int poff[MPC_MLP_MAX_LAYERS];      // Pt_k, k = 0 .. L-1: float offset from the start of the point matrices
    int coff[MPC_MLP_MAX_LAYERS + 1];  // Ct_k, k = 1 .. L
    int gboff[MPC_MLP_MAX_LAYERS];     // gb_k inside the bias slots
    int tbase[MPC_MLP_MAX_LAYERS];     // first tile of gW_k
    int mat_floats;                    // all point matrices together
    int tile[PG_MAX_TILES];            // k | row tile << 8 | column tile << 16
};

template <bool WL, int MAXT>
__global__ void __launch_bounds__(256) nn_param_grad_kernel(MlpDesc m, PgDesc g, long N, int ns, int nc, const float *x, const float *u,
                                                            const float *gF, const float *gf, float *partials, int TS, int ZS,
                                                            int wave_floats)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float *wts = stage_weights<WL>(m, lds);
    const int wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
    float *stage = lds + (WL ? m.total : 0);
    float *tauS = stage + wave * wave_floats, *zb = tauS + 16 * TS;
    float *mat = zb + (m.L > 1 ? m.L - 1 : 1) * 16 * ZS, *gbS = mat + g.mat_floats;
    float *red = stage + nwave * wave_floats;                   // [nwave][256]: the block's sum of one tile
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int n = ns + nc, L = m.L, NC = g.NC, JS = g.JS, NTJ = NC >> 4;
    const bool sigmoid = m.act == MPC_ACT_SIGMOID;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) acc[t] = zero4;
    for (int e = lane; e < g.gbtotal; e += 64) gbS[e] = 0.f;
    wave_sync();
    const long groups = (N + 15) / 16, stride = (long)gridDim.x * nwave;
    for (long grp = (long)blockIdx.x * nwave + wave; grp < groups; grp += stride) {
        const long p0 = grp * 16;
        const long pt = (p0 + r < N) ? p0 + r : N - 1;
        for (int f0 = 4 * q; f0 < m.wp[0]; f0 += 16) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int fe = f0 + v;
                tauS[r * TS + fe] = fe < ns ? x[pt * ns + fe] : (fe < n ? u[pt * nc + (fe - ns)] : 0.f);
            }
        }
        wave_sync();
        (void)mlp_forward<true, 1>(m, wts, tauS, TS, zb, ZS, q, r);    // the hidden activations of the sixteen points
        for (int pp = 0; pp < 16; ++pp) {
            if (p0 + pp >= N) break;
            const float *tau = tauS + pp * TS;
            // Pt_0 = [ I | tau ]
            {
                float *P0 = mat + g.poff[0];
                for (int e = lane; e < m.wp[0] * NC; e += 64) {
                    const int i = e / NC, j = e - i * NC;
                    P0[i * JS + j] = i < n ? (j == i ? 1.f : (j == n ? tau[i] : 0.f)) : 0.f;
                }
            }
            // Ct_L = [ gF - gf tau' | gf ]
            {
                float *CL = mat + g.coff[L];
                const float *gFp = gF + (p0 + pp) * ns * n, *gfp = gf + (p0 + pp) * ns;
                for (int e = lane; e < m.wp[L] * NC; e += 64) {
                    const int i = e / NC, j = e - i * NC;
                    float val = 0.f;
                    if (i < ns && j <= n) {
                        const float gi = gfp[i];
                        val = j < n ? fmaf(-gi, tau[j], gFp[i * n + j]) : gi;
                    }
                    CL[i * JS + j] = val;
                }
            }
            wave_sync();
            // forward chain: Pt_k = [ diag(s_k) W_{k-1} P_{k-1} | a_k ],  k = 1 .. L-1
            for (int k = 1; k < L; ++k) {
                const int nout_t = m.wp[k] >> 4, nin_t = m.wp[k - 1] >> 4, ld = m.wp[k - 1] + 4;
                const float *zrow = zb + (k - 1) * 16 * ZS + pp * ZS;
                const float *W = wts + m.woff[k - 1];
                const float *Pprev = mat + g.poff[k - 1];
                float *Pk = mat + g.poff[k];
                for (int to = 0; to < nout_t; ++to) {
                    const f32x4 zq = *reinterpret_cast<const f32x4 *>(zrow + 16 * to + 4 * q);
                    const f32x4 s = slope_fn(zq, m.act);
                    for (int tj = 0; tj < NTJ; ++tj) {
                        const int col = 16 * tj + r;
                        f32x4 gv;
                        if (k == 1) {
#pragma unroll
                            for (int v = 0; v < 4; ++v) {
                                const float wv = W[(16 * to + 4 * q + v) * ld + (col < m.wp[0] ? col : 0)];
                                gv[v] = col < m.wp[0] ? s[v] * wv : 0.f;
                            }
                        } else {
                            f32x4 a0 = zero4, a1 = zero4, a2 = zero4, a3 = zero4;
                            const float *wrow = W + (16 * to + r) * ld + 4 * q;
                            const float *brow = Pprev + (4 * q) * JS + col;
                            for (int ti = 0; ti < nin_t; ++ti) {
                                const f32x4 a = *reinterpret_cast<const f32x4 *>(wrow + 16 * ti);
                                const float *bp = brow + 16 * ti * JS;
                                const float b0 = bp[0], b1 = bp[JS], b2 = bp[2 * JS], b3 = bp[3 * JS];
                                a0 = mfma(a[0], b0, a0);
                                a1 = mfma(a[1], b1, a1);
                                a2 = mfma(a[2], b2, a2);
                                a3 = mfma(a[3], b3, a3);
                            }
                            gv = ((a0 + a1) + (a2 + a3)) * s;
                        }
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int row = 16 * to + 4 * q + v;
                            Pk[row * JS + col] = col == n ? (row < m.w[k] ? zq[v] : 0.f) : gv[v];
                        }
                    }
                }
                wave_sync();
            }
            // backward chain: [ cP_k | ca_k ] = W_k' Ct_{k+1}, then Ct_k in place,  k = L-1 .. 1
            for (int k = L - 1; k >= 1; --k) {
                const int nrow_t = m.wp[k] >> 4, ncon_t = m.wp[k + 1] >> 4, ld = m.wp[k] + 4;
                const float *zrow = zb + (k - 1) * 16 * ZS + pp * ZS;
                const float *W = wts + m.woff[k];
                const float *Cn = mat + g.coff[k + 1], *Pk = mat + g.poff[k];
                float *Ck = mat + g.coff[k];
                for (int ti = 0; ti < nrow_t; ++ti) {
                    const f32x4 zq = *reinterpret_cast<const f32x4 *>(zrow + 16 * ti + 4 * q);
                    const f32x4 s = slope_fn(zq, m.act);
                    f32x4 part = zero4;
                    for (int tj = 0; tj < NTJ; ++tj) {
                        const int col = 16 * tj + r;
                        f32x4 a0 = zero4, a1 = zero4, a2 = zero4, a3 = zero4;
                        const float *arow = W + (4 * q) * ld + 16 * ti + r;       // W_k'[16 ti + r][4q + v] = W_k[4q + v][16 ti + r]
                        const float *brow = Cn + (4 * q) * JS + col;
                        for (int to = 0; to < ncon_t; ++to) {
                            const float *ap = arow + 16 * to * ld, *bp = brow + 16 * to * JS;
                            const float w0 = ap[0], w1 = ap[ld], w2 = ap[2 * ld], w3 = ap[3 * ld];
                            const float b0 = bp[0], b1 = bp[JS], b2 = bp[2 * JS], b3 = bp[3 * JS];
                            a0 = mfma(w0, b0, a0);
                            a1 = mfma(w1, b1, a1);
                            a2 = mfma(w2, b2, a2);
                            a3 = mfma(w3, b3, a3);
                        }
                        const f32x4 d = (a0 + a1) + (a2 + a3);
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int row = 16 * ti + 4 * q + v;
                            const float pv = Pk[row * JS + col];
                            part[v] = col < n ? fmaf(d[v], pv, part[v]) : part[v];
                            Ck[row * JS + col] = s[v] * d[v];
                        }
                    }
                    if (sigmoid) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            float a = part[v];
                            a += __shfl_xor(a, 1);
                            a += __shfl_xor(a, 2);
                            a += __shfl_xor(a, 4);
                            a += __shfl_xor(a, 8);
                            part[v] = a;
                        }
                        wave_sync();
                        if (r == (n & 15)) {
#pragma unroll
                            for (int v = 0; v < 4; ++v) {
                                const int row = 16 * ti + 4 * q + v;
                                Ck[row * JS + n] = fmaf(1.f - 2.f * zq[v], part[v], Ck[row * JS + n]);
                            }
                        }
                    }
                }
                wave_sync();
            }
            // gW_k += Ct_{k+1} Pt_k' (tile t: register quadruple t), gb_k += column n of Ct_{k+1}
#pragma unroll
            for (int t = 0; t < MAXT; ++t) {
                if (t < g.ntiles) {
                    const int code = g.tile[t], k = code & 255, to = (code >> 8) & 255, ti = code >> 16;
                    const float *arow = mat + g.coff[k + 1] + (16 * to + r) * JS + 4 * q;
                    const float *brow = mat + g.poff[k] + (16 * ti + r) * JS + 4 * q;
                    f32x4 c = acc[t];
                    for (int kk = 0; kk < NTJ; ++kk) {
                        const f32x4 a = *reinterpret_cast<const f32x4 *>(arow + 16 * kk);
                        const f32x4 b = *reinterpret_cast<const f32x4 *>(brow + 16 * kk);
                        c = mfma(a[0], b[0], c);
                        c = mfma(a[1], b[1], c);
                        c = mfma(a[2], b[2], c);
                        c = mfma(a[3], b[3], c);
                    }
                    acc[t] = c;
                }
            }
            for (int k = 0; k < L; ++k) {
                const float *Cn = mat + g.coff[k + 1];
                for (int row = lane; row < m.wp[k + 1]; row += 64) gbS[g.gboff[k] + row] += Cn[row * JS + n];
            }
            wave_sync();
        }
    }
    // the block's partial: its wavefronts added in wave order
    __syncthreads();
    float *part = partials + (long)blockIdx.x * g.psize;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        if (t < g.ntiles) {
            reinterpret_cast<f32x4 *>(red)[wave * 64 + lane] = acc[t];
            __syncthreads();
            if (wave == 0) {
                f32x4 s = reinterpret_cast<const f32x4 *>(red)[lane];
                for (int w = 1; w < nwave; ++w) s += reinterpret_cast<const f32x4 *>(red)[w * 64 + lane];
                reinterpret_cast<f32x4 *>(part)[t * 64 + lane] = s;
            }
            __syncthreads();
        }
    }
    for (int e = threadIdx.x; e < g.gbtotal; e += blockDim.x) {
        float s = 0.f;
        for (int w = 0; w < nwave; ++w) s += stage[w * wave_floats + (gbS - tauS) + e];
        part[g.ntiles * 256 + e] = s;
    }
}

struct PgFinalArgs {
    int L, ntiles, psize, nparts;
    int w[MPC_MLP_MAX_LAYERS + 1], wp[MPC_MLP_MAX_LAYERS + 1];
    int tbase[MPC_MLP_MAX_LAYERS], gboff[MPC_MLP_MAX_LAYERS];
    const float *partials;
    float *gW[MPC_MLP_MAX_LAYERS], *gb[MPC_MLP_MAX_LAYERS];
};

// one thread per returned entry: the blocks' partials added in block order (nparts = 0: zeros)
__global__ void __launch_bounds__(256) nn_param_grad_final_kernel(PgFinalArgs a)
{
    long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < a.L; ++k) {
        const int out = a.w[k + 1], in = a.w[k];
        const long cnt = (long)out * in + out;
        if (e < cnt) {
            int slot;
            float *dst;
            if (e < (long)out * in) {
                const int o = (int)(e / in), i = (int)(e - (long)o * in);
                const int t = a.tbase[k] + (o >> 4) * (a.wp[k] >> 4) + (i >> 4);
                slot = t * 256 + ((((o & 15) >> 2) * 16 + (i & 15)) << 2) + (o & 3);      // accumulator layout: lane (q, r), register v
                dst = a.gW[k] + e;
            } else {
                const int o = (int)(e - (long)out * in);
                slot = a.ntiles * 256 + a.gboff[k] + o;
                dst = a.gb[k] + o;
            }
            float s = 0.f;
            for (int b = 0; b < a.nparts; ++b) s += a.partials[(long)b * a.psize + slot];
            *dst = s;
            return;
        }
        e -= cnt;
    }
}

// the layout of a point's matrices, the tile list, the launch shape; false when the network is outside this kernel
struct PgPlan {
    PgDesc g;
    int TS, ZS, wave_floats, nw;
    bool wl;
    size_t lds;
    int64_t packed_bytes;              // the packed network's share of the workspace (the partials follow, 256-byte aligned)
};

bool pg_plan(const MlpDesc &d, int ns, int nc, PgPlan &pl)
{
    const int *wp = d.wp, L = d.L;
    PgDesc &g = pl.g;
    g.NC = pad16(ns + nc + 1);
    g.JS = g.NC + 4;
    int nt = 0, off = 0, gb = 0;
    for (int k = 0; k < L; ++k) {
        g.tbase[k] = nt;
        for (int to = 0; to < (wp[k + 1] >> 4); ++to)
            for (int ti = 0; ti < (wp[k] >> 4); ++ti) {
                if (nt >= PG_MAX_TILES) return false;
                g.tile[nt++] = k | (to << 8) | (ti << 16);
            }
        g.poff[k] = off;
        off += wp[k] * g.JS;
        g.gboff[k] = gb;
        gb += wp[k + 1];
    }
    g.coff[0] = 0;
    for (int k = 1; k <= L; ++k) {
        g.coff[k] = off;
        off += wp[k] * g.JS;
    }
    for (int t = nt; t < PG_MAX_TILES; ++t) g.tile[t] = 0;
    g.ntiles = nt;
    g.gbtotal = gb;
    g.psize = nt * 256 + gb;
    g.mat_floats = off;
    pl.TS = wp[0] + 4;
    pl.ZS = max_hidden_pad(d) + 4;
    pl.wave_floats = 16 * pl.TS + (L > 1 ? L - 1 : 1) * 16 * pl.ZS + off + gb;
    const size_t wbytes = (size_t)d.total * 4, per_wave = (size_t)(pl.wave_floats + 256) * 4;       // (+ the wave's row of `red`)
    const int nw_g = (int)(LDS_MAX / per_wave);
    const int nw_l = wbytes <= WEIGHTS_IN_LDS_MAX && wbytes < LDS_MAX ? (int)((LDS_MAX - wbytes) / per_wave) : 0;
    if (nw_g < 1) return false;
    auto cap = [](int v) { return v > PG_MAX_WAVES ? PG_MAX_WAVES : v; };
    pl.wl = nw_l >= 1 && cap(nw_l) >= cap(nw_g) - 1 && 2 * cap(nw_l) >= cap(nw_g);      // staged weights unless they cost half the waves
    pl.nw = cap(pl.wl ? nw_l : nw_g);
    pl.lds = (pl.wl ? wbytes : 0) + pl.nw * per_wave;
    pl.packed_bytes = ((int64_t)d.total * 4 + 256 + 255) & ~(int64_t)255;
    return true;
}

int pg_blocks(long N, int nw)
{
    const long groups = (N + 15) / 16, b = (groups + nw - 1) / nw;
    return (int)(b > PG_MAX_BLOCKS ? PG_MAX_BLOCKS : b);
}

// the packed network, then one partial per block (at least one: an empty call still has a workspace)
int64_t pg_workspace_bytes(const PgPlan &pl, long N)
{
    const int blocks = pg_blocks(N, pl.nw);
    return pl.packed_bytes + (int64_t)(blocks > 0 ? blocks : 1) * pl.g.psize * 4;
}
