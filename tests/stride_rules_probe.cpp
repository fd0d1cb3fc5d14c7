// stride_rules_probe.cpp -- host-only, for tests/test_stride_rules_host.py: what every support rule of csrc/lqr_rules.hip and every
// route entry answers for a made-up float32 problem whose eight strides and seven base pointers are moved ONE AT A TIME.  Nothing is
// launched and no pointer is dereferenced.  One call per line of standard input, 21 integers:
//   ns nc T B bounds has_f   dC_st dC_sb dc_st dc_sb dF_st dF_sb df_st df_sb (elements added to the dense stride)
//   oC oc oF of ox_init ocur_x ocur_u (bytes added to the 16-byte aligned base)
// and one JSON object per line back: "rules" (the predicates as they stand), "step" (StepRoute of impl 0, 3, 5, 7, 8, 9: code, kernel,
// pad16), "kkt" (mpc_lqr_kkt_fused_kernel_route of kernel 0..7 and MPC_KKT_PREFER_NARROW), "grads" (mpc_lqr_kkt_grads_route).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../mpc.pytorch_amd/csrc/lqr_common.h"

using namespace mpclqr;

enum { N_ARGS = 21 };

static void probe(const long *a)
{
    const int ns = (int)a[0], nc = (int)a[1], T = (int)a[2], B = (int)a[3], n = ns + nc;
    char *const base = (char *)(uintptr_t)(1 << 20), *const ws = (char *)(uintptr_t)(1 << 24), *const g = (char *)(uintptr_t)(1 << 22);
    mpc_lqr_problem p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.T = T; p.ns = ns; p.nc = nc; p.dtype = MPC_F32;
    p.C_st = (int64_t)B * n * n + a[6]; p.C_sb = n * n + a[7]; p.c_st = B * n + a[8]; p.c_sb = n + a[9];
    p.F_st = (int64_t)B * ns * n + a[10]; p.F_sb = ns * n + a[11];
    p.C = base + a[14]; p.c = base + a[15]; p.F = base + a[16];
    if (a[5]) { p.f = base + a[17]; p.f_st = B * ns + a[12]; p.f_sb = ns + a[13]; }
    p.x_init = base + a[18]; p.cur_x = base + a[19]; p.cur_u = base + a[20];
    mpc_lqr_options o;
    memset(&o, 0, sizeof(o));
    o.bound_mode = (int)a[4]; o.lo_s = -1; o.hi_s = 1; o.max_linesearch_iter = 10; o.linesearch_decay = 0.2; o.delta_u = 0.0 / 0.0; o.pnqp_iter = 20;
    o.flags = MPC_OPT_C_SYMMETRIC;
    mpc_lqr_outputs out;
    memset(&out, 0, sizeof(out));
    out.new_x = out.new_u = out.costs = out.old_costs = out.full_du_norm = out.alpha_du_norm = out.alphas = g;
    out.qp_iters = out.status = (int32_t *)g;
    const StepParams<float> sp = make_params<float>(&p, &o, &out);
    const float *gf = (const float *)g, *wf = (const float *)ws;
    printf("{\"rules\": {\"dpp16\": %d, \"dpp16_pad\": %d, \"mfma40\": %d, \"mfma40_pad\": %d, \"mfma40_pad16\": %d, \"mfma40_narrow\": %d, "
           "\"kkt_dpp16\": %d, \"kkt_fused_dpp16\": %d, \"kkt_fused_dpp16_pad\": %d, \"kkt_fused_mfma40\": %d, \"kkt_fused_mfma40_pad\": %d, "
           "\"kkt_fused_mfma40_pad16\": %d, \"kkt_fused_mfma40_narrow\": %d, \"kkt_fused_mfma40_narrow16\": %d}",
           (int)dpp16_supported(sp), (int)dpp16_pad_supported(sp), (int)mfma40_supported(sp), (int)mfma40_pad_supported(sp),
           (int)mfma40_pad16_supported(sp), (int)mfma40_narrow_supported(sp), (int)kkt_dpp16_supported(sp, gf, gf, gf, gf, gf),
           (int)kkt_fused_dpp16_supported(sp, gf, gf, gf, gf, wf), (int)kkt_fused_dpp16_pad_supported(sp, wf),
           (int)kkt_fused_mfma40_supported(sp, gf, gf, gf, gf, wf), (int)kkt_fused_mfma40_pad_supported(sp, wf),
           (int)kkt_fused_mfma40_pad16_supported(sp, wf), (int)kkt_fused_mfma40_narrow_supported(sp, wf),
           (int)kkt_fused_mfma40_narrow16_supported(sp, wf));
    const int64_t full = mpc_lqr_workspace_bytes(&p);
    printf(", \"step\": {");
    const int impls[] = {0, 3, 5, 7, 8, 9};
    for (int i = 0; i < 6; ++i) {
        const StepRoute r = step_route(sp, &p, impls[i], 3, ws, full);
        int ring = -1;
        const int entry = mpc_lqr_step_route(&p, &o, &out, ws, full, impls[i], &ring);
        printf("%s\"%d\": [%d, %d, %d, %d, %d]", i ? ", " : "", impls[i], r.code, r.kernel, (int)r.pad16, entry,
               mpc_lqr_impl_supported(&p, &o, impls[i]));
    }
    printf("}, \"kkt\": {");
    const int kernels[] = {0, 1, 2, 3, 4, 5, 6, 7, MPC_KKT_PREFER_NARROW};
    for (int i = 0; i < 9; ++i) {
        const int64_t kb = mpc_lqr_kkt_fused_kernel_workspace_bytes(&p, &o, kernels[i]);
        const int rc = mpc_lqr_kkt_fused_kernel_route(&p, &o, kernels[i], g, g, g, g, g, a[5] ? g : nullptr, g, g, g, (const int32_t *)g, ws, kb);
        printf("%s\"%d\": %d", i ? ", " : "", kernels[i], rc);
    }
    printf("}, \"grads\": %d}\n", mpc_lqr_kkt_grads_route(&p, g, g, g, g, g, g, g, a[5] ? g : nullptr, g));
}

int main()
{
    long a[N_ARGS];
    for (int j = 0; scanf("%ld", &a[j]) == 1;)
        if (++j == N_ARGS) { probe(a); j = 0; }
    return 0;
}
