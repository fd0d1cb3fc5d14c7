// lqr_mfma40.hip -- gfx950 binding of the register-resident MFMA sweep for n_state = 32, n_ctrl = 8
// (lqr_mfma40_body.h): one wavefront per problem and per workgroup, a 3-slot LDS-DMA sweep ring (36 KiB: 4 wavefronts per
// CU) or a 2-slot one (26 KiB: 6 per CU).
#include <string>
#include "lqr_common.h"

// Compiled eleven times (Makefile): the step kernels on the three-slot sweep ring (launch_step_mfma40), the same with
// -DMPC_MFMA40_SWEEP_NSTAGE=2 (launch_step_mfma40_ring2), with -DMPC_MFMA40_KKT the fused KKT backward (three slots); the padded
// instantiation -DMPC_MFMA40_PAD=4 | 16 on two slots, as step kernels and as fused KKT backward (four objects); and the padded step
// kernels on one state tile, -DMPC_MFMA40_XT=1 with either granule, on three slots (launch_step_mfma40_narrow4 / _narrow16), and
// that tile's fused KKT backward the same way (launch_kkt_fused_mfma40_narrow4 / _narrow16).
#ifndef MPC_MFMA40_SWEEP_NSTAGE
#define MPC_MFMA40_SWEEP_NSTAGE 3              // (lqr_mfma40_body.h: why the sweep looks two timesteps ahead)
#endif
// state tiles of 16 rows (lqr_mfma40_body.h): 2 = the 32/8 kernel, 1 = its narrow instantiation (n_state <= 16, padded only)
#ifndef MPC_MFMA40_XT
#define MPC_MFMA40_XT 2
#endif
#define MPC_MFMA40_NS_ (16 * MPC_MFMA40_XT)
#define MPC_MFMA40_N_ (MPC_MFMA40_NS_ + 8)
// a sweep stage C | F | record and a pricing-rollout stage C | F | K | record: 12032 and 13056 B at two state tiles, 4352 and 4864 at one
#define MPC_MFMA40_STAGE_ (4 * MPC_MFMA40_N_ * MPC_MFMA40_N_ + 4 * MPC_MFMA40_NS_ * MPC_MFMA40_N_ + 512)
#define MPC_MFMA40_RSTAGE_ (MPC_MFMA40_STAGE_ + 32 * MPC_MFMA40_NS_)
// pass 2's stage of the fused backward, F | K | record | V: 10752 B at two state tiles
#define MPC_MFMA40_KSTAGE_ (4 * MPC_MFMA40_NS_ * MPC_MFMA40_N_ + 32 * MPC_MFMA40_NS_ + 512 + 1024 * MPC_MFMA40_XT * MPC_MFMA40_XT)
// the sweep's slots or the pricing rollout's two, + the layout-turn words; the fused backward's second ring (31.5 KiB) lies inside
// its three sweep slots
#define MPC_MFMA40_LDS_STEP ((MPC_MFMA40_SWEEP_NSTAGE * MPC_MFMA40_STAGE_ > 2 * MPC_MFMA40_RSTAGE_ ? MPC_MFMA40_SWEEP_NSTAGE * MPC_MFMA40_STAGE_ : 2 * MPC_MFMA40_RSTAGE_) + 512)
// (the padded fused backward sweeps on two slots: its second ring alone sets the size then)
#if defined(MPC_MFMA40_KKT) && MPC_MFMA40_LDS_STEP < 3 * MPC_MFMA40_KSTAGE_
#define MPC_MFMA40_LDS (3 * MPC_MFMA40_KSTAGE_)
#else
#define MPC_MFMA40_LDS MPC_MFMA40_LDS_STEP
#endif
#define MPC_WV_STAGE_BYTES MPC_MFMA40_LDS
#include "wv_gfx950.h"

namespace mpclqr {
namespace wv {
MPC_DEV float readlane(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
MPC_DEV bool uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }
// sum over the four 16-lane rows, result in every lane: two row swaps (gfx950 v_permlane{16,32}_swap), no LDS
MPC_DEV float sum_rows(float x)
{
    auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    const float s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
// rows 0 and 1 (lanes 0..15, 16..31) of x, each copied to all four rows: the same two row swaps
MPC_DEV void rows01(float x, float &r0, float &r1)
{
    auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);     // rows {0,1,0,1}
    auto b = __builtin_amdgcn_permlane16_swap(a[0], a[0], false, false);
    r0 = __uint_as_float(b[0]);
    r1 = __uint_as_float(b[1]);
}
// lo = {a.row0, b.row0, a.row2, b.row2}, hi = {a.row1, b.row1, a.row3, b.row3} (rows of 16 lanes): v_permlane16_swap
// exchanges the odd rows of its first operand with the even rows of its second
MPC_DEV void swap16(float a, float b, float &lo, float &hi)
{
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    lo = __uint_as_float(r[0]);
    hi = __uint_as_float(r[1]);
}
// lo = {a.lanes 0..31, b.lanes 0..31}: v_permlane32_swap exchanges the upper half of its first operand with the lower half of
// its second (the other result, the two upper halves, is not wanted where this is used)
MPC_DEV float lower_halves(float a, float b)
{
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]);
}
// the sum over lanes 0..7 of a row, in lanes 0..7 of it (lanes 8..15: their own): the first three of row_sum's four steps --
// for the box QP's vectors, which live in lanes 0..7 and whose sums are read in lane 0 (wv::first_lane)
MPC_DEV float row_sum8(float x)
{
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x141, 0xf, 0xf, true));   // row_half_mirror
    return x;
}
// lane 0's truth value, as a wave-uniform one (uniform() says "every lane holds this"; this says "lane 0 decides")
MPC_DEV bool first_lane(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }
MPC_DEV float rcp_fast(float x) { return __builtin_amdgcn_rcpf(x); }     // v_rcp_f32 as it comes: 1 ulp
MPC_DEV float rcp(float x)
{
    float r = __builtin_amdgcn_rcpf(x);
    return fmaf(fmaf(-x, r, 1.f), r, r);     // one Newton step: <= 1 ulp
}
// ---- HBM -> LDS staging: what only this kernel uses (the array and the shared primitives: wv_gfx950.h, part 3) ----
MPC_DEV void dma16(const void *g, unsigned off)
{
    __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(g_stage + off), 16, 0, 0);
}
// dma16_at (wv_gfx950.h) of a block read exactly once per launch: the non-temporal policy (C_AUX, aux bit 1)
template <int IMM> MPC_DEV void dma16_once_at(const void *g, unsigned off)
{
    static_assert(IMM >= 0 && IMM < 4096, "13-bit signed immediate");
    __builtin_amdgcn_global_load_lds((glb_void_t *)g, (lds_void_t *)(g_stage + off), 16, IMM, C_AUX);
}
// ---- the padded instantiation's staging (lqr_mfma40_body.h, PADK; dma_buf and dma4_if: wv_gfx950.h) ------------------------------
// a wave-uniform pointer / word the compiler has moved to vector registers, back in scalar ones (two / one v_readfirstlane): the dword build's
// C block address is computed on the vector ALU next to the timestep counter, and a buffer descriptor made from it was then wrapped in a
// readfirstlane LOOP -- per gather, 25 a timestep (round 6)
MPC_DEV const void *uniform_ptr(const void *q)
{
    const unsigned long long v = (unsigned long long)q;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (const void *)(((unsigned long long)hi << 32) | (unsigned long long)lo);
}
MPC_DEV unsigned uniform_u32(unsigned x) { return (unsigned)__builtin_amdgcn_readfirstlane((int)x); }
// a dword to `base + voff` through a raw buffer of `nbytes`: a lane whose voff lies beyond the buffer stores nothing
MPC_DEV void st_buf(float *base, unsigned nbytes, unsigned voff, float v)
{
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, (int)nbytes, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)voff, 0, 0);
}
// ... where `base` is the same for every lane of the wave (a row of one problem and timestep): the address is wave-uniform, but the compiler
// computes it next to the timestep counter on the vector ALU and then wraps the store in a readfirstlane loop -- see uniform_ptr.  (st_buf
// itself stays general: the copy-out of a parked trajectory addresses a different row per lane.)
MPC_DEV void st_buf_u(float *base, unsigned nbytes, unsigned voff, float v)
{
    st_buf((float *)uniform_ptr(base), uniform_u32(nbytes), voff, v);
}
}  // namespace wv
}  // namespace mpclqr

#include "lqr_mfma40_body.h"
// (the fused KKT builds, whose array may be set by pass 2's ring instead; the step builds assert equality further down)
static_assert(mpclqr::mfma40::LDS_TOTAL <= MPC_MFMA40_LDS, "the staging array is smaller than the body's rings");

// ---- Which build is this? -------------------------------------------------------------------------------------------------------------
// The shapes and sweep rings the Makefile builds (FLAGS_lqr_mfma40*), each with the launchers of its two objects: without -DMPC_MFMA40_KKT
// an object holds the step kernel's three modes and exports MPC_MFMA40_STEP_LAUNCH, with it the fused KKT backward's two kernels, no step
// kernel, and MPC_MFMA40_KF_LAUNCH.  Any other combination of the flags is an error.  What else the step launcher has to know about its
// build -- the shape, its rule (lqr_rules.hip), what it checks beyond the rule, its texts -- it reads off the body's constants: Build, next to it.
#define MPC_MFMA40_ON(xt, ring) (MPC_MFMA40_XT == xt && MPC_MFMA40_SWEEP_NSTAGE == ring)
#if !defined(MPC_MFMA40_PAD) && MPC_MFMA40_ON(2, 3)          // lqr_mfma40.o, lqr_mfma40_kkt.o: the exact shape on three sweep slots
#define MPC_MFMA40_STEP_LAUNCH launch_step_mfma40
#define MPC_MFMA40_KF_LAUNCH launch_kkt_fused_mfma40
#elif !defined(MPC_MFMA40_PAD) && MPC_MFMA40_ON(2, 2) && !defined(MPC_MFMA40_KKT)          // lqr_mfma40_ring2.o: ... on two (the step alone)
#define MPC_MFMA40_STEP_LAUNCH launch_step_mfma40_ring2
#elif MPC_MFMA40_PAD == 4 && MPC_MFMA40_ON(2, 2)             // lqr_mfma40_pad4.o, _padkkt.o: padded, dword gathers, two slots
#define MPC_MFMA40_STEP_LAUNCH launch_step_mfma40_pad4
#define MPC_MFMA40_KF_LAUNCH launch_kkt_fused_mfma40_pad
#elif MPC_MFMA40_PAD == 16 && MPC_MFMA40_ON(2, 2)            // lqr_mfma40_pad16.o, _pad16kkt.o: ... 16-byte gathers
#define MPC_MFMA40_STEP_LAUNCH launch_step_mfma40_pad16
#define MPC_MFMA40_KF_LAUNCH launch_kkt_fused_mfma40_pad16
#elif MPC_MFMA40_PAD == 4 && MPC_MFMA40_ON(1, 3)             // lqr_mfma40_narrow4.o, _narrow4kkt.o: padded on ONE state tile, three slots
#define MPC_MFMA40_STEP_LAUNCH launch_step_mfma40_narrow4
#define MPC_MFMA40_KF_LAUNCH launch_kkt_fused_mfma40_narrow4
#elif MPC_MFMA40_PAD == 16 && MPC_MFMA40_ON(1, 3)            // lqr_mfma40_narrow16.o, _narrow16kkt.o
#define MPC_MFMA40_STEP_LAUNCH launch_step_mfma40_narrow16
#define MPC_MFMA40_KF_LAUNCH launch_kkt_fused_mfma40_narrow16
#else
#error "lqr_mfma40.hip: a combination of MPC_MFMA40_PAD / _XT / _SWEEP_NSTAGE / _KKT that the Makefile does not build"
#endif

namespace mpclqr {
#ifdef MPC_MFMA40_KKT
namespace {
static_assert(mfma40::KLDS_TOTAL <= MPC_MFMA40_LDS && mfma40::LDS_TOTAL <= MPC_MFMA40_LDS, "the fused KKT kernel's rings do not fit");
// MODE 0: no bounds; 1: controls on a bound pinned in the nested solve
template <int MODE> __global__ void __launch_bounds__(64, 1) lqr_kkt_fused_mfma40_kernel(StepParams<float> p, float *K, float *k,
                                                                                        mfma40::KktArgs40 kx)
{
    mfma40::kkt_fused_wave<MODE>(p, K, k, kx);
}
}  // namespace

// the nested step with lambda and dlambda riding along (one launch), then the outer products (kkt_wave.hip)
int MPC_MFMA40_KF_LAUNCH(const StepParams<float> &p_in, const float *dl_dx, const float *dl_du, float *dC, float *dc, float *dF,
                         float *df, float *dx_init, float *dx_out, float *du_out, float *ws, float decay, int max_ls, hipStream_t st)
{
    using namespace rules;
    StepParams<float> p = p_in;
    const long TB = (long)p.T * p.B;
    // the workspace as lqr_params.h describes it for this build's state tiles (and lqr_rules.hip sizes it)
    constexpr int XT = mfma40::XT;
    constexpr int at_K = kf40_off(XT, KF40_K), at_k = kf40_off(XT, KF40_k), at_V = kf40_off(XT, KF40_V), at_vg = kf40_off(XT, KF40_VG),
                  at_dx = kf40_off(XT, KF40_DX), at_du = kf40_off(XT, KF40_DU);
    float *K = ws + TB * at_K, *k = ws + TB * at_k, *V = ws + TB * at_V, *vg = ws + TB * at_vg, *dx = ws + TB * at_dx, *du = ws + TB * at_du;
    static_assert(at_du + mfma40::NC == kf40_off(XT, KF40_END), "the carving ends where the workspace's size does");
    static_assert(kf40_words(XT, KF40_K) == mfma40::NC * mfma40::NS && kf40_words(XT, KF40_k) == mfma40::NC &&
                  kf40_words(XT, KF40_DX) == mfma40::NS, "the workspace's parts are the body's");
    if (dx_out && du_out) { dx = dx_out; du = du_out; }
    p.new_x = dx;
    p.new_u = du;
    p.ls_decay = decay;
    p.max_ls = max_ls;
    p.old_costs = nullptr;
    p.qp_iters = nullptr;
    p.c_symmetric = true;
    p.zero_mask = nullptr;
    p.has_delta = 0;
    mfma40::KktArgs40 kx;
    kx.dl_dx = dl_dx; kx.dl_du = dl_du; kx.dF = dF; kx.df = df; kx.dx_init = dx_init; kx.Vws = V; kx.vgws = vg;
    if (p.bound_mode != MPC_BOUND_NONE) hipLaunchKernelGGL((lqr_kkt_fused_mfma40_kernel<1>), dim3(p.B), dim3(64), 0, st, p, K, k, kx);
    else hipLaunchKernelGGL((lqr_kkt_fused_mfma40_kernel<0>), dim3(p.B), dim3(64), 0, st, p, K, k, kx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error((std::string("lqr_kkt_fused_mfma40_kernel: ") + hipGetErrorString(e)).c_str());
        return MPC_E_LAUNCH;
    }
    return launch_kkt_outer(p, dx, du, dC, dc, dF, st);
}
#else
namespace {
// the step launcher's texts, by shape
struct StepTexts { const char *refused, *missing, *misaligned, *launch; };
struct Build {
    enum Shape { EXACT, PADDED, NARROW };
    static constexpr Shape SHAPE = !mfma40::PADK ? EXACT : mfma40::XT == 2 ? PADDED : NARROW;
    static constexpr bool GATHERS16 = mfma40::PADK && mfma40::PADG == 16;
    static constexpr StepTexts TEXTS[3] = {
        {"mfma40: needs fp32, n_state = 32, n_ctrl = 8, 16-byte aligned blocks", "mfma40: K / k / new_x / new_u missing",
         "mfma40: outputs must be 16-byte aligned", "lqr_step_mfma40_kernel: "},
        {"mfma40 (padded): needs fp32, n_state <= 32, n_ctrl <= 8, max_linesearch_iter <= 16, no simulator", "mfma40 (padded): K / k / new_x / new_u missing",
         "mfma40 (padded): the gain workspace must be 16-byte aligned", "lqr_step_mfma40_kernel (padded): "},
        {"mfma40 (narrow): needs fp32, n_state <= 16, n_ctrl <= 8, max_linesearch_iter <= 16, no simulator", "mfma40 (narrow): K / k / new_x / new_u missing",
         "mfma40 (narrow): the gain workspace must be 16-byte aligned", "lqr_step_mfma40_kernel (narrow): "}};
    static bool takes(const StepParams<float> &p)
    {
        return SHAPE == NARROW ? mfma40_narrow_supported(p) : SHAPE == PADDED ? mfma40_pad_supported(p) : mfma40_supported(p);
    }
    // what has to sit on 16 bytes beyond the rule: the exact kernel's outputs, or the padded kernels' own gains in the workspace (p.K / p.k:
    // [T,B,8,32] or [T,B,8,16] / [T,B,8]; p.K_user / p.k_user are the caller's) -- and the narrow kernel's record
    static bool misaligned(const StepParams<float> &p)
    {
        const uintptr_t more = SHAPE == EXACT ? (uintptr_t)p.new_x | (uintptr_t)p.new_u : SHAPE == NARROW ? (uintptr_t)p.Kk : 0;
        return (((uintptr_t)p.K | (uintptr_t)p.k | more) & 15) != 0;
    }
};

static_assert(mfma40::LDS_TOTAL == MPC_MFMA40_LDS, "the step kernels reserve their rings and nothing more");
// MODE: 0 unconstrained, 1 unconstrained + u_zero_I, 2 box-constrained (pnqp8 in the sweep)
template <int MODE> __global__ void __launch_bounds__(64, 1) lqr_step_mfma40_kernel(StepParams<float> p)
{
    mfma40::step_wave<MODE>(p, p.K, p.k);
}
}  // namespace

int MPC_MFMA40_STEP_LAUNCH(const StepParams<float> &p, hipStream_t st)
{
    constexpr StepTexts tx = Build::TEXTS[Build::SHAPE];
    if (!Build::takes(p)) { set_last_error(tx.refused); return MPC_E_DIMS; }
    // (the padded kernel's 16-byte build is only ever handed calls that pass this, capi.hip: StepRoute::pad16; the narrow one asks)
    if (Build::SHAPE == Build::NARROW && Build::GATHERS16 && !mfma40_pad16_supported(p)) { set_last_error("mfma40 (narrow): 16-byte gathers need n_state, n_ctrl multiples of 4 and 16-byte aligned blocks"); return MPC_E_ARG; }
    if (!p.K || !p.k || (!p.sweep_only && (!p.new_x || !p.new_u))) { set_last_error(tx.missing); return MPC_E_NULL; }
    if (Build::misaligned(p)) { set_last_error(tx.misaligned); return MPC_E_ARG; }
    if (p.bound_mode != MPC_BOUND_NONE)
        hipLaunchKernelGGL(lqr_step_mfma40_kernel<2>, dim3(p.B), dim3(64), 0, st, p);
    else if (p.zero_mask)
        hipLaunchKernelGGL(lqr_step_mfma40_kernel<1>, dim3(p.B), dim3(64), 0, st, p);
    else
        hipLaunchKernelGGL(lqr_step_mfma40_kernel<0>, dim3(p.B), dim3(64), 0, st, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error((std::string(tx.launch) + hipGetErrorString(e)).c_str());
        return MPC_E_LAUNCH;
    }
    return MPC_OK;
}
#endif

}  // namespace mpclqr
