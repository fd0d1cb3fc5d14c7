// lqr_common.h -- shared device-side parameter blocks for the gfx950 LQR kernels.
//
// The algorithm these kernels implement is the batched LQR step of
// locuslab/mpc.pytorch (mpc/lqr_step.py, mpc/pnqp.py, mpc/util.py); each kernel
// cites the reference lines it replaces.  Nothing here is translated from the
// reference's Python: the reference issues ~13 ATen launches per timestep, these
// kernels own the whole time loop with one wavefront per problem.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mpc_lqr.h"
#include "lqr_params.h"

namespace mpclqr {

void set_last_error(const char *msg);

// the kernels behind mpc_lqr_step: the values of its `impl` argument (include/mpc_lqr.h)
enum { MPC_IMPL_AUTO = 0, MPC_IMPL_GENERIC = 1, MPC_IMPL_MFMA16 = 2, MPC_IMPL_DPP16 = 3, MPC_IMPL_TINY = 4, MPC_IMPL_MFMA40 = 5,
       MPC_IMPL_WAVE1 = 6, MPC_IMPL_MFMA40_PAD = 7, MPC_IMPL_DPP16_PAD = 8,
       MPC_IMPL_MFMA40_NARROW = 9,         // (9: forced only -- impl 0 never chooses it; the narrow instantiation of 7 for n_state <= 16)
       MPC_IMPL_WAVE1_CARRY = 10 };        // (10: forced only; the instantiation of 6 for a simulator behind MPC_ENV_CTRL_CARRY, n_state = 4 / 6)

// Which kernel takes one step call and where its pieces live in the workspace (capi.hip: step_route decides, step_impl executes,
// the queries mpc_lqr_step_route / mpc_lqr_qp_record read it off).  Host only.
struct StepRoute {
    int code; const char *msg;     // code != 0: refused, with mpc_lqr_step's code and text (a string literal)
    int kernel;                    // MPC_IMPL_* 1..10: the kernel that takes the call
    int phase;                     // the generic kernels: 3 = sweep + rollout, 1 = sweep, 2 = rollout
    int ring;                      // 0, or the sweep ring of the 12/4 / 32/8 kernel (2 / 4, 2 / 3)
    bool pad16;                    // padded 32/8 and its narrow instantiation: 16-byte gathers
    bool needs_resolve;            // the generic re-solve of the problems flagged MPC_ST_C_ASYMMETRIC follows the launch
    // where things live in the workspace (byte offsets, -1 = not there)
    int64_t K_off, k_off;          // gains the kernel parks there (the caller's out->K / out->k otherwise)
    int64_t Kk_off, status_off;    // the kernel's own record; the status words of a caller that passes none
    int64_t qp_off, qp_st, qp_sb;  // the k_t record a later step may start from (mpc_lqr_qp_record; qp_off < 0: none), element strides
};
template <typename real>
StepRoute step_route(const StepParams<real> &sp, const mpc_lqr_problem *p, int impl, int phase_mask, const void *workspace,
                     int64_t workspace_bytes);

// Which fused kernel takes one KKT backward (capi.hip: kkt_fused_route decides, mpc_lqr_kkt_fused executes, mpc_lqr_kkt_fused_route
// and the entry's two queries read it off).  Host only.
struct KktPointers {               // the entry's pointers: inspected for NULL and alignment, never dereferenced
    const void *dl_dx, *dl_du, *dC, *dc, *dF, *df, *dx_init, *dx_out, *du_out, *workspace;
};
struct KktRoute {
    int code; const char *msg;     // code != 0: refused, with mpc_lqr_kkt_fused's code and text (a string literal) ...
    bool no_kernel;                // ... because no fused kernel takes these sizes, flags or views: the three-call route's case
    int kernel;                    // MPC_KKT_* (include/mpc_lqr.h); MPC_KKT_NONE with code 0: an empty batch
    int64_t bytes;                 // the workspace that kernel needs
};
KktRoute kkt_fused_route(const StepParams<float> &sp, const mpc_lqr_problem *p, const KktPointers &a, int64_t workspace_bytes);
// ... for a call that asks for a kernel: 0 = the line above, an exact MPC_KKT_* code, or the family MPC_KKT_PREFER_NARROW
KktRoute kkt_fused_route_kernel(const StepParams<float> &sp, const mpc_lqr_problem *p, const KktPointers &a, int64_t workspace_bytes,
                                int kernel);

// generic path (lqr_generic.hip)
template <typename real> int launch_step_generic(const StepParams<real> &p, int phase_mask, hipStream_t st);
template <typename real> int launch_pnqp(int B, int n, const real *H, const real *q, const real *lo,
                                         const real *hi, const real *x0, int n_iter, real *x,
                                         uint8_t *If_out, int *iters, int *status, real *Hfree,
                                         real *LU, int *pivots, hipStream_t st);
template <typename real> int launch_traj_cost(const StepParams<real> &p, real *x, real *cost, hipStream_t st);
template <typename real> int launch_kkt_grads(const StepParams<real> &p, const real *dx, const real *du,
                                              const real *dl_dx, const real *dl_du, real *dC, real *dc,
                                              real *dF, real *df, real *dx_init, hipStream_t st);
template <typename real> int launch_kkt_prepare(int B, int T, int ns, int nc, const real *dl_dx,
                                                const real *dl_du, const real *u_star, int bound_mode,
                                                real lo_s, real hi_s, const real *lo, const real *hi,
                                                real *negr, uint8_t *mask, hipStream_t st);
template <typename real> int launch_select_best(int B, int T, int ns, int nc, int first, real eps,
                                                const real *x, const real *u, const real *costs,
                                                const real *du_norm, real *bx, real *bu, real *bc,
                                                real *bd, void *flags, void *host_flags, int host_tag, const int *status,
                                                hipStream_t st);
template <typename real> int launch_du_norm_reference(int T, int B, int nc, const real *u, const real *new_u, real *out, hipStream_t st);
template <typename real> int launch_env_linearize(const EnvDesc<real> &env, long N, const real *x, const real *u,
                                                  real *F, real *f, hipStream_t st);
// its backward with respect to the simulator's parameters (env_param_grad.hip): gparams [env_np(kind)], ws = workspace of
// env_param_grad_workspace_bytes(N) bytes, 8-byte aligned
int64_t env_param_grad_workspace_bytes(int64_t N);
template <typename real> int launch_env_param_grad(const EnvDesc<real> &env, long N, const real *x, const real *u,
                                                   const real *gF, const real *gf, real *gparams, double *ws, hipStream_t st);
size_t generic_lds_bytes(int ns, int nc, size_t elem);
// the slew-rate augmentation (aC, ac, aF, af) of p's (C, c, F, f) in one launch (slew_augment.hip)
template <typename real> int launch_slew_augment(const mpc_lqr_problem *p, double gamma, real *aC, real *ac, real *aF, real *af, hipStream_t st);

// 4-problems-per-wave DPP path for n_state = 12, n_ctrl = 4, f32 (lqr_dpp16.hip: the launchers, one per compilation of that file --
// Makefile; lqr_rules.hip: every *_supported and *_workspace_bytes of this family and of the 32/8 one below, compiled once)
bool dpp16_supported(const StepParams<float> &p);
int launch_step_dpp16(const StepParams<float> &p, hipStream_t st);
int launch_step_dpp16_ring2(const StepParams<float> &p, hipStream_t st);    // the same kernels on a 2-slot sweep ring (two waves per SIMD)
bool dpp16_pad_supported(const StepParams<float> &p);                          // (round 6) the PADDED instantiation: any n_state <= 12, n_ctrl <= 4, no alignment asked
int launch_step_dpp16_res(const StepParams<float> &p, hipStream_t st);      // mode 0 on the 2-slot ring with a share of F resident in LDS (one wave per SIMD)
int launch_step_dpp16_pad(const StepParams<float> &p, hipStream_t st);
bool kkt_dpp16_supported(const StepParams<float> &p, const float *dx, const float *du, const float *dl_dx,
                         const float *dC, const float *dF);
int launch_kkt_dpp16(const StepParams<float> &p, const float *dx, const float *du, const float *dl_dx, float *dC,
                     float *dc, float *dF, float *df, float *dx_init, hipStream_t st);

// the whole KKT backward in one launch, n_state = 12, n_ctrl = 4, T <= 64, f32, symmetric C (lqr_dpp16.hip)
bool kkt_fused_dpp16_supported(const StepParams<float> &p, const float *dl_dx, const float *dl_du, const float *dC,
                               const float *dF, const float *ws);
int64_t kkt_fused_dpp16_workspace_bytes(int T, int B);
// ... and its PADDED instantiation: any n_state <= 12, n_ctrl <= 4, no alignment asked (lqr_dpp16.hip, -DMPC_DPP16_PAD_KKT; the same workspace)
bool kkt_fused_dpp16_pad_supported(const StepParams<float> &p, const float *ws);
int launch_kkt_fused_dpp16_pad(const StepParams<float> &p, const float *dl_dx, const float *dl_du, float *dC, float *dc, float *dF,
                               float *df, float *dx_init, float *dx_out, float *du_out, float *ws, float decay, int max_ls,
                               hipStream_t st);
int launch_kkt_fused_dpp16(const StepParams<float> &p, const float *dl_dx, const float *dl_du, float *dC, float *dc, float *dF,
                           float *df, float *dx_init, float *dx_out, float *du_out, float *ws, float decay, int max_ls,
                           hipStream_t st);

// one lane per problem, n_ctrl = 1, n_state <= 6, f32 / f64 (lqr_tiny.hip)
bool tiny_supported(int ns, int nc);
template <typename real> int launch_step_tiny(const StepParams<real> &p, hipStream_t st);
// a 16-lane row per problem, the same shapes, f32, the problem in LDS (lqr_wave1.hip)
bool wave1_supported(const StepParams<float> &p);
long wave1_lds_bytes(const StepParams<float> &p);        // per wavefront (four problems)
int launch_step_wave1(const StepParams<float> &p, hipStream_t st);
// ... and its CARRY instantiation: a simulator behind MPC_ENV_CTRL_CARRY, n_state = 4 / 6, and nothing else (lqr_wave1_carry.hip)
bool wave1_carry_supported(const StepParams<float> &p);
long wave1_carry_lds_bytes(const StepParams<float> &p);  // per wavefront (four problems)
int launch_step_wave1_carry(const StepParams<float> &p, hipStream_t st);

// wave-per-problem trajectory kernel for 16 < n <= 64, f32 (kkt_wave.hip)
bool traj_wave_supported(const StepParams<float> &p);
int launch_traj_wave(const StepParams<float> &p, float *x, hipStream_t st);
// costate + outer-product kernels of the KKT backward for n <= 64, f32 (kkt_wave.hip)
bool kkt_wave_supported(const StepParams<float> &p, const float *dx, const float *du, const float *dl_dx, const float *dC,
                        const float *dF);
int launch_kkt_wave(const StepParams<float> &p, const float *dx, const float *du, const float *dl_dx, float *dC,
                    float *dc, float *dF, float *df, float *dx_init, hipStream_t st);
// ... the same two kernels in float64, 2 <= n <= 64 (kkt_wave64.hip); forced only: mpc_lqr_kkt_grads_kernel(MPC_KKT_GRADS_WAVE64).
// Every pointer on 8 bytes; what is also on the 16-byte grid moves 16 bytes a lane, everything else 4.
bool kkt_wave64_sizes(int ns, int nc);
int launch_kkt_wave64(const StepParams<double> &p, const double *dx, const double *du, const double *dl_dx, double *dC,
                      double *dc, double *dF, double *df, double *dx_init, hipStream_t st);

// the costate recursion alone, parked in a compact [T-1,B,2 ns] area (kkt_wave.hip), and the batch-summed gradients of a shared
// C, c, F, f built on it (kkt_shared.hip): outputs [T,n,n], [T,n], [T-1,ns,n], [T-1,ns], each may be NULL
int launch_kkt_costates(const StepParams<float> &p, const float *dx, const float *du, const float *dl_dx, float *park, float *dx_init,
                        hipStream_t st);
int kkt_shared_partials(int T, int B);
int64_t kkt_shared_workspace_bytes(int T, int B, int ns, int nc);
int launch_kkt_shared(const StepParams<float> &p, const float *dx, const float *du, const float *dl_dx, float *sum_dC, float *sum_dc,
                      float *sum_dF, float *sum_df, float *dx_init, void *workspace, hipStream_t st);

int launch_kkt_outer(const StepParams<float> &p, const float *dx, const float *du, float *dC, float *dc, float *dF, hipStream_t st);

// register-resident MFMA step for n_state = 32, n_ctrl = 8, f32 (lqr_mfma40.hip)
bool mfma40_supported(const StepParams<float> &p);
int launch_step_mfma40(const StepParams<float> &p, hipStream_t st);            // three-slot sweep ring (36 KiB per wave: four per CU)
int launch_step_mfma40_ring2(const StepParams<float> &p, hipStream_t st);      // two slots (26 KiB: six per CU), see capi.hip
// the same kernel for ANY n_state <= 32, n_ctrl <= 8 (round 4): tau padded to [x(32); u(8)] by the staging gathers
// (lqr_mfma40_body.h, PADK); p.K / p.k = the kernel's own padded gains [T,B,8,32] / [T,B,8], p.K_user / p.k_user the caller's
bool mfma40_pad_supported(const StepParams<float> &p);
bool mfma40_pad16_supported(const StepParams<float> &p);                        // ... with 16-byte gathers (n_state, n_ctrl multiples of 4)
int launch_step_mfma40_pad4(const StepParams<float> &p, hipStream_t st);
int launch_step_mfma40_pad16(const StepParams<float> &p, hipStream_t st);
// ... and its NARROW instantiation for n_state <= 16 (-DMPC_MFMA40_XT=1: one state tile, tau padded to [x(16); u(8)]); p.K / p.k =
// the kernel's own gains [T,B,8,16] / [T,B,8] inside the padded kernel's workspace layout
bool mfma40_narrow_supported(const StepParams<float> &p);                       // the padded predicate with n_state <= 16
int launch_step_mfma40_narrow4(const StepParams<float> &p, hipStream_t st);
int launch_step_mfma40_narrow16(const StepParams<float> &p, hipStream_t st);
// the KKT backward of that shape: the nested step with both costates riding along + kkt_outer_kernel (lqr_mfma40.hip, -DMPC_MFMA40_KKT)
bool kkt_fused_mfma40_supported(const StepParams<float> &p, const float *dl_dx, const float *dl_du, const float *dC,
                                const float *dF, const float *ws);
int64_t kkt_fused_mfma40_workspace_bytes(int T, int B);
// ... and its PADDED instantiation: any n_state <= 32, n_ctrl <= 8 (lqr_mfma40.hip, -DMPC_MFMA40_KKT -DMPC_MFMA40_PAD=4; the same workspace)
bool kkt_fused_mfma40_pad_supported(const StepParams<float> &p, const float *ws);
bool kkt_fused_mfma40_pad16_supported(const StepParams<float> &p, const float *ws);          // (n_state, n_ctrl multiples of 4, 16-byte aligned C / F)
int launch_kkt_fused_mfma40_pad16(const StepParams<float> &p, const float *dl_dx, const float *dl_du, float *dC, float *dc, float *dF,
                                  float *df, float *dx_init, float *dx_out, float *du_out, float *ws, float decay, int max_ls,
                                  hipStream_t st);
int launch_kkt_fused_mfma40_pad(const StepParams<float> &p, const float *dl_dx, const float *dl_du, float *dC, float *dc, float *dF,
                                float *df, float *dx_init, float *dx_out, float *du_out, float *ws, float decay, int max_ls,
                                hipStream_t st);
int launch_kkt_fused_mfma40(const StepParams<float> &p, const float *dl_dx, const float *dl_du, float *dC, float *dc, float *dF,
                            float *df, float *dx_init, float *dx_out, float *du_out, float *ws, float decay, int max_ls,
                            hipStream_t st);
// ... and the padded instantiation on ONE state tile (-DMPC_MFMA40_XT=1, lqr_mfma40_narrow4kkt.o / _narrow16kkt.o): the padded predicates with
// n_state <= 16, and a workspace of their own -- K [T,B,8,16] | k | V [T,B,256] | v,g [T,B,32] | (dx [T,B,16] | du): 448 floats a problem-step
bool kkt_fused_mfma40_narrow_supported(const StepParams<float> &p, const float *ws);
bool kkt_fused_mfma40_narrow16_supported(const StepParams<float> &p, const float *ws);
int64_t kkt_fused_mfma40_narrow_workspace_bytes(int T, int B);
int launch_kkt_fused_mfma40_narrow16(const StepParams<float> &p, const float *dl_dx, const float *dl_du, float *dC, float *dc, float *dF,
                                     float *df, float *dx_init, float *dx_out, float *du_out, float *ws, float decay, int max_ls,
                                     hipStream_t st);
int launch_kkt_fused_mfma40_narrow4(const StepParams<float> &p, const float *dl_dx, const float *dl_du, float *dC, float *dc, float *dF,
                                    float *df, float *dx_init, float *dx_out, float *du_out, float *ws, float decay, int max_ls,
                                    hipStream_t st);

// NNDynamics inside the kernels: rollout / line search and Jacobian on MFMA, 16 problems per wave (nn_dynamics.hip)
int nn_budget(const mpc_mlp_dynamics *net, int ns, int nc);     // bit 0: the rollout kernels take this network, bit 1: the linearisation ones
int64_t nn_workspace_bytes(const mpc_mlp_dynamics *net);         // the packed network (+ alignment slack); 0: illegal layer count
int launch_nn_rollout(const StepParams<float> &p, const mpc_mlp_dynamics *net, void *workspace, int64_t bytes, hipStream_t st);
int launch_nn_linearize(const mpc_mlp_dynamics *net, long N, int ns, int nc, const float *x, const float *u, float *F,
                        float *f, void *workspace, int64_t bytes, hipStream_t st);
// ... into the slew-rate augmentation's layout: z [N,nc+ns] = (u_prev, x), aF [N,na,na+nc], af [N,na], na = ns + nc (same kernels)
int launch_nn_linearize_carry(const mpc_mlp_dynamics *net, long N, int ns, int nc, const float *z, const float *u, float *aF,
                              float *af, void *workspace, int64_t bytes, hipStream_t st);
// ... and the linearisation's weight gradient (nn_param_grad.h); nn_budget bit 2 says whether it takes the network
int64_t nn_param_grad_workspace_bytes(const mpc_mlp_dynamics *net, int64_t N);     // -1: outside the kernel
int launch_nn_param_grad(const mpc_mlp_dynamics *net, long N, int ns, int nc, const float *x, const float *u, const float *gF,
                         const float *gf, const mpc_mlp_param_grads *out, void *workspace, int64_t bytes, hipStream_t st);

// ... and the same network in float64 on plain FMA, one wavefront per problem / point (nn_dynamics64.hip): rollout / line search and the
// dense linearisation; no augmented-layout linearisation
int nn64_budget(const mpc_mlp_dynamics *net, int ns, int nc);   // bits 0 and 1 as nn_budget
int64_t nn64_workspace_bytes(const mpc_mlp_dynamics *net);       // 0: illegal layer count
int launch_nn64_rollout(const StepParams<double> &p, const mpc_mlp_dynamics *net, void *workspace, int64_t bytes, hipStream_t st);
int launch_nn64_linearize(const mpc_mlp_dynamics *net, long N, int ns, int nc, const double *x, const double *u, double *F, double *f,
                          void *workspace, int64_t bytes, hipStream_t st);
// ... and the linearisation's weight gradient in float64, one point a block and pass (nn_param_grad64.h): sigmoid / relu, no
// ctrl_carry, a complete description
int nn64_param_grad_supported(const mpc_mlp_dynamics *net, int ns, int nc);                 // 1 / 0
int64_t nn64_param_grad_workspace_bytes(const mpc_mlp_dynamics *net, int64_t N);            // -1: outside the kernel
int launch_nn64_param_grad(const mpc_mlp_dynamics *net, long N, int ns, int nc, const double *x, const double *u, const double *gF,
                           const double *gf, const mpc_mlp_param_grads *out, void *workspace, int64_t bytes, hipStream_t st);

// fused MFMA path for n <= 16, f32 (lqr_mfma16.hip)
bool mfma16_supported(const StepParams<float> &p);
int launch_step_mfma16(const StepParams<float> &p, hipStream_t st);
bool mfma16_supported(const StepParams<double> &p);          // (round 5) the same kernel on v_mfma_f64_16x16x4_f64
int launch_step_mfma16(const StepParams<double> &p, hipStream_t st);

}  // namespace mpclqr
