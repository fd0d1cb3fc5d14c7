// lqr_rules.hip -- the host-side rules of the 12/4 (lqr_dpp16.hip) and 32/8 (lqr_mfma40.hip) families: which call a kernel takes and
// what workspace its fused KKT backward needs.  Host only, compiled once; the two kernel files are compiled once per variant
// (Makefile) and hold launchers only.  capi.hip's tables (step_kernels[], kkt_order[]) and the launchers ask these.
#include "lqr_common.h"

namespace mpclqr {
namespace {
bool al16(const void *q) { return ((uintptr_t)q & 15) == 0; }
// a block the exact kernels stream in 16-byte DMA granules: its start on 16 bytes, its strides on four floats
bool al16(const void *q, long st, long sb) { return al16(q) && st % 4 == 0 && sb % 4 == 0; }
// bound rows (and mask bytes) read as dwords through the scalar path
bool bounds_al4(const StepParams<float> &p) { return p.bound_mode != MPC_BOUND_TENSOR || ((((uintptr_t)p.lo | (uintptr_t)p.hi) & 3) == 0); }
// rows of C and F and the x | u boundary on 16 bytes: what 16-byte gathers ask of a padded shape
bool gathers16(const StepParams<float> &p)
{
    return p.ns % 4 == 0 && p.nc % 4 == 0 && al16(p.C) && (p.T == 1 || al16(p.F)) && p.C_st % 4 == 0 && p.C_sb % 4 == 0 &&
           p.F_st % 4 == 0 && p.F_sb % 4 == 0;
}
}  // namespace

// ---- 12/4: the step ------------------------------------------------------------------------------------------------------------
bool dpp16_supported(const StepParams<float> &p)
{
    // 16-byte DMA granules: every block the kernel streams must start on a 16-byte boundary
    if (!(p.ns == 12 && p.nc == 4 && p.T >= 1 && p.max_ls >= 1 && p.max_ls <= 16)) return false;
    if (!al16(p.C, p.C_st, p.C_sb) || !al16(p.c, p.c_st, p.c_sb)) return false;
    if (p.T > 1 && !al16(p.F, p.F_st, p.F_sb)) return false;
    if (p.f && !al16(p.f, p.f_st, p.f_sb)) return false;
    if (!al16(p.cur_x) || !al16(p.cur_u)) return false;
    if (p.bound_mode == MPC_BOUND_TENSOR && (!al16(p.lo) || !al16(p.hi))) return false;
    if (p.zero_mask && (uintptr_t)p.zero_mask % 4 != 0) return false;
    return true;
}
// the PADDED instantiation (dword gathers: float arrays are 4-byte aligned by construction; u_zero_I is read byte-wise.  12/4 itself is
// welcome too: blocks or strides that are not 16-byte aligned, which the exact kernel refuses)
bool dpp16_pad_supported(const StepParams<float> &p)
{
    return p.ns >= 1 && p.ns <= 12 && p.nc >= 1 && p.nc <= 4 && p.T >= 1 && p.max_ls >= 1 && p.max_ls <= 16 && !p.env.kind;
}

// ---- 12/4: the KKT backward ----------------------------------------------------------------------------------------------------
bool kkt_dpp16_supported(const StepParams<float> &p, const float *dx, const float *du, const float *dl_dx,
                         const float *dC, const float *dF)
{
    if (!(p.ns == 12 && p.nc == 4 && p.T >= 1)) return false;
    if (!al16(p.C, p.C_st, p.C_sb) || !al16(p.c, p.c_st, p.c_sb)) return false;
    if (p.T > 1 && !al16(p.F, p.F_st, p.F_sb)) return false;
    return al16(p.cur_x) && al16(p.cur_u) && al16(dx) && al16(du) && al16(dl_dx) && al16(dC) && (p.T == 1 || al16(dF));
}
// the fused one (any horizon since round 4: T > 64 on the LONG instantiation)
bool kkt_fused_dpp16_supported(const StepParams<float> &p, const float *dl_dx, const float *dl_du, const float *dC,
                               const float *dF, const float *ws)
{
    if (!(p.ns == 12 && p.nc == 4 && p.T >= 1)) return false;
    if (!al16(p.C, p.C_st, p.C_sb) || !al16(p.c, p.c_st, p.c_sb)) return false;
    if (p.T > 1 && !al16(p.F, p.F_st, p.F_sb)) return false;
    if (p.bound_mode == MPC_BOUND_TENSOR && (!al16(p.lo) || !al16(p.hi))) return false;
    // (p.zero_mask / p.has_delta: the forward's u_zero_I and delta_u, which the backward does not use -- mpc/lqr_step.py:322-340;
    // launch_kkt_fused_dpp16 clears them)
    return al16(p.cur_x) && al16(p.cur_u) && al16(dl_dx) && al16(dl_du) && al16(dC) && al16(ws) && (p.T == 1 || al16(dF));
}
// ... and its PADDED instantiation (round 6): any n_state <= 12, n_ctrl <= 4, no alignment asked of the caller's blocks (dword gathers
// and dword stores); the workspace -- the library's own layout, padded to 12/4 -- on 16 bytes
bool kkt_fused_dpp16_pad_supported(const StepParams<float> &p, const float *ws)
{
    return p.ns >= 1 && p.ns <= 12 && p.nc >= 1 && p.nc <= 4 && p.T >= 1 && al16(ws);
}
// floats per problem-step: (V | v) 96, (lambda | g) 24, and beyond 64 timesteps the gain record 64
int64_t kkt_fused_dpp16_workspace_bytes(int T, int B)
{
    return (int64_t)T * B * (rules::DPP16_KF_VBLK + 24 + (T > rules::DPP16_RG_STEPS ? 64 : 0)) * 4 + 64;
}

// ---- 32/8: the step ------------------------------------------------------------------------------------------------------------
bool mfma40_supported(const StepParams<float> &p)
{
    // (the record's per-lane pointers step by 32-bit byte counts, lqr_mfma40_body.h: Stream)
    auto fits = [](long elems) { return elems >= 0 && elems < (1L << 30); };
    return p.ns == 32 && p.nc == 8 && p.T >= 1 && p.max_ls >= 1 && p.max_ls <= 16 && !p.env.kind &&
           fits(p.c_st) && fits(p.f ? p.f_st : 0) && fits((long)p.B * 64) &&
           !(p.bound_mode != MPC_BOUND_NONE && p.zero_mask) &&
           al16(p.C) && al16(p.c) && (p.T == 1 || al16(p.F)) && al16(p.cur_x) && al16(p.cur_u) && p.C_st % 4 == 0 && p.C_sb % 4 == 0 &&
           p.c_st % 4 == 0 && p.c_sb % 4 == 0 && p.F_st % 4 == 0 && p.F_sb % 4 == 0 &&
           (!p.f || al16(p.f, p.f_st, p.f_sb)) && al16(p.x_init) &&
           (!p.zero_mask || ((uintptr_t)p.zero_mask & 3) == 0) && bounds_al4(p);
}
// the PADDED instantiation: any n_state <= 32, n_ctrl <= 8 in float32: every staging access is a dword, nothing but 4-byte alignment
// is asked for
bool mfma40_pad_supported(const StepParams<float> &p)
{
    return p.ns >= 1 && p.ns <= 32 && p.nc >= 1 && p.nc <= 8 && p.T >= 1 && p.max_ls >= 1 && p.max_ls <= 16 && !p.env.kind &&
           !(p.bound_mode != MPC_BOUND_NONE && p.zero_mask) && bounds_al4(p);
}
// ... with 16-byte gathers (asked on top of the line above, or of the narrow one)
bool mfma40_pad16_supported(const StepParams<float> &p) { return gathers16(p); }
// ... and on ONE state tile
bool mfma40_narrow_supported(const StepParams<float> &p) { return mfma40_pad_supported(p) && p.ns <= 16; }

// ---- 32/8: the fused KKT backward ----------------------------------------------------------------------------------------------
bool kkt_fused_mfma40_supported(const StepParams<float> &p, const float *dl_dx, const float *dl_du, const float *dC,
                                const float *dF, const float *ws)
{
    if (!(p.ns == 32 && p.nc == 8 && p.T >= 1)) return false;
    if (!al16(p.C, p.C_st, p.C_sb) || !al16(p.c, p.c_st, p.c_sb)) return false;
    if (p.T > 1 && !al16(p.F, p.F_st, p.F_sb)) return false;
    if (!bounds_al4(p)) return false;
    if (p.env.kind) return false;           // (zero_mask / has_delta: the forward's, dropped by the launcher -- mpc/lqr_step.py:322-340)
    if (p.c_st >= (1L << 30) || (long)p.B * 64 >= (1L << 30)) return false;       // (32-bit record steps, lqr_mfma40_body.h: Stream)
    return al16(p.cur_x) && al16(p.cur_u) && al16(dl_dx) && al16(dl_du) && al16(dC) && al16(ws) && (p.T == 1 || al16(dF));
}
// the PADDED instantiation (round 6): any n_state <= 32, n_ctrl <= 8, dword gathers -- nothing but 4-byte alignment asked of the caller's
// blocks; the workspace (the library's padded layout) on 16
bool kkt_fused_mfma40_pad_supported(const StepParams<float> &p, const float *ws)
{
    return p.ns >= 1 && p.ns <= 32 && p.nc >= 1 && p.nc <= 8 && p.T >= 1 && !p.env.kind && al16(ws) && bounds_al4(p);
}
// ... with 16-byte gathers: a quarter of the staging instructions
bool kkt_fused_mfma40_pad16_supported(const StepParams<float> &p, const float *ws) { return kkt_fused_mfma40_pad_supported(p, ws) && gathers16(p); }
// ... and both on ONE state tile, in a workspace packed for it.  Forced only (capi.hip: kkt_order)
bool kkt_fused_mfma40_narrow_supported(const StepParams<float> &p, const float *ws) { return kkt_fused_mfma40_pad_supported(p, ws) && p.ns <= 16; }
bool kkt_fused_mfma40_narrow16_supported(const StepParams<float> &p, const float *ws) { return kkt_fused_mfma40_pad16_supported(p, ws) && p.ns <= 16; }
// the workspace (lqr_params.h: rules::kf40_off) on two state tiles and on one, + 64 bytes of slack
int64_t kkt_fused_mfma40_workspace_bytes(int T, int B)
{
    constexpr int words = rules::kf40_off(2, rules::KF40_END);
    return (int64_t)T * B * words * 4 + 64;
}
int64_t kkt_fused_mfma40_narrow_workspace_bytes(int T, int B)
{
    constexpr int words = rules::kf40_off(1, rules::KF40_END);
    return (int64_t)T * B * words * 4 + 64;
}

}  // namespace mpclqr
