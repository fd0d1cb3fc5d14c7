// step_route_probe.cpp -- host-only: prints the whole StepRoute (csrc/capi.hip: step_route) of made-up step calls, one JSON object
// per line, for tests/test_step_route_host.py and tests/test_step_route_full.py.  Nothing is launched and no pointer is dereferenced.
//   step_route_probe  (ns nc f64 T B bounds mask max_ls sweep_only gains workspace align impl status sim carry linearize phase)...
// or, without arguments, the same eighteen integers per call from standard input.
// bounds: 0 none, 1 scalar, 2 tensor; gains: 0 none, 1 out->K and out->k, 2 out->K alone; workspace: 0 none, 1 full
// (mpc_lqr_workspace_bytes, aligned), 2 the same 4 bytes off, 3 the padded gains' bytes only (T B (256 + 8) floats); align: 16 or 4 (every
// block of the problem 4 bytes off); status: out->status given; sim: 0 none, 1..3 the simulator kind as true_dynamics, with carry
// (MPC_ENV_CTRL_CARRY) and linearize; phase: 3 the step, 1 / 2 the sweep and rollout entries.
// "entry" is what mpc_lqr_step_route itself answers for a step (the argument checks in front of the route included), with its text.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../mpc.pytorch_amd/csrc/lqr_common.h"

using namespace mpclqr;

enum { N_ARGS = 18 };

template <typename real>
static void probe(const int *a)
{
    const int ns = a[0], nc = a[1], T = a[3], B = a[4], n = ns + nc, phase = a[17];
    char *const ptr = (char *)(uintptr_t)((1 << 20) + (a[11] == 16 ? 0 : 4)), *const ws = (char *)(uintptr_t)(1 << 24);
    mpc_lqr_problem p;
    memset(&p, 0, sizeof(p));
    p.B = B; p.T = T; p.ns = ns; p.nc = nc; p.dtype = a[2] ? MPC_F64 : MPC_F32;
    p.x_init = p.C = p.c = p.F = p.f = p.cur_x = p.cur_u = ptr;
    p.C_st = (int64_t)B * n * n; p.C_sb = n * n; p.c_st = B * n; p.c_sb = n;
    p.F_st = (int64_t)B * ns * n; p.F_sb = ns * n; p.f_st = B * ns; p.f_sb = ns;
    mpc_lqr_options o;
    memset(&o, 0, sizeof(o));
    o.bound_mode = a[5]; o.lo_s = -1; o.hi_s = 1; o.max_linesearch_iter = a[7]; o.linesearch_decay = 0.2; o.delta_u = 0.0 / 0.0; o.pnqp_iter = 20;
    if (a[5] == 2) o.lo = o.hi = (char *)(uintptr_t)(1 << 20);
    if (a[6]) o.zero_mask = (const uint8_t *)(uintptr_t)(1 << 20);
    if (a[8]) o.flags = MPC_OPT_SWEEP_ONLY;
    mpc_env_dynamics env;
    memset(&env, 0, sizeof(env));
    if (a[14]) {
        env.kind = a[14] | (a[15] ? MPC_ENV_CTRL_CARRY : 0); env.linearize = a[16]; env.params = (char *)(uintptr_t)(1 << 20);
        env.dt = 0.05; env.u_max = 2.0;
        o.true_dynamics = &env;
    }
    mpc_lqr_outputs out;
    memset(&out, 0, sizeof(out));
    out.new_x = out.new_u = out.costs = out.old_costs = out.full_du_norm = out.alpha_du_norm = out.alphas = ptr;
    out.qp_iters = (int32_t *)ptr;
    if (a[13]) out.status = (int32_t *)ptr;
    if (a[9]) out.K = ptr;
    if (a[9] == 1) out.k = ptr;
    const int64_t full = mpc_lqr_workspace_bytes(&p), gains_only = (int64_t)T * B * (256 + 8) * 4;
    const void *w = a[10] == 0 ? nullptr : (a[10] == 2 ? ws + 4 : ws);
    const int64_t bytes = a[10] == 0 ? 0 : (a[10] == 3 ? gains_only : full);
    const StepRoute r = step_route(make_params<real>(&p, &o, &out), &p, a[12], phase, w, bytes);
    printf("{\"code\": %d, \"kernel\": %d, \"phase\": %d, \"ring\": %d, \"pad16\": %d, \"needs_resolve\": %d, \"K_off\": %lld, \"k_off\": %lld, "
           "\"Kk_off\": %lld, \"status_off\": %lld, \"qp\": [%lld, %lld, %lld], \"workspace_bytes\": %lld, \"msg\": ",
           r.code, r.kernel, r.phase, r.ring, (int)r.pad16, (int)r.needs_resolve, (long long)r.K_off, (long long)r.k_off, (long long)r.Kk_off,
           (long long)r.status_off, (long long)r.qp_off, (long long)r.qp_st, (long long)r.qp_sb, (long long)full);
    if (r.code) printf("\"%s\"", r.msg); else printf("null");        // (no text of the library holds a quote or a backslash)
    if (phase == 3) {
        int ring = -1;
        const int rc = mpc_lqr_step_route(&p, &o, &out, w, bytes, a[12], &ring);
        printf(", \"entry\": [%d, %d, \"%s\"]", rc, ring, rc < 0 ? mpc_lqr_last_error() : "");
    }
    printf("}\n");
}

static void probe_one(const int *a)
{
    if (a[2]) probe<double>(a); else probe<float>(a);
}

int main(int argc, char **argv)
{
    int a[N_ARGS];
    for (int i = 1; i + N_ARGS <= argc; i += N_ARGS) {
        for (int j = 0; j < N_ARGS; ++j) a[j] = atoi(argv[i + j]);
        probe_one(a);
    }
    if (argc == 1)
        for (int j = 0; scanf("%d", &a[j]) == 1;)
            if (++j == N_ARGS) { probe_one(a); j = 0; }
    return 0;
}
