// time_step_route.cpp -- host-only: nanoseconds per call of mpc_lqr_step_route, which runs in front of every mpc_lqr_step launch and is
// never cached, for three made-up calls (no pointer is dereferenced, nothing is launched; docs/history/r22.md has the numbers):
//   the 12/4 headline step (T = 50, B = 4096, no bounds), a box-constrained 32/8 step (T = 64, B = 1024) and a 3/1 step with the pendulum
//   as true_dynamics, linearised in the kernel (T = 20, B = 1024) -- each under impl 0 with a full workspace and no out->K / out->k.
// Build against the library to be timed (the compiler of csrc/Makefile), run it a few times, compare the medians it prints:
//   hipcc -std=c++17 -O2 -x hip --cuda-host-only tools/time_step_route.cpp -o time_step_route -L<dir> -lmpc_lqr_hip -Wl,-rpath,<dir>
//   ./time_step_route [calls per repeat = 200000] [repeats = 11]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/mpc_lqr.h"

struct Call {
    const char *name;
    int ns, nc, T, B, bounds, sim, linearize;
};

int main(int argc, char **argv)
{
    const long calls = argc > 1 ? atol(argv[1]) : 200000;
    const int repeats = argc > 2 ? atoi(argv[2]) : 11;
    const Call table[] = {{"12/4 headline", 12, 4, 50, 4096, MPC_BOUND_NONE, 0, 0},
                          {"32/8 box", 32, 8, 64, 1024, MPC_BOUND_SCALAR, 0, 0},
                          {"3/1 pendulum", 3, 1, 20, 1024, MPC_BOUND_SCALAR, MPC_ENV_PENDULUM, 1}};
    char *const ptr = (char *)(uintptr_t)(1 << 20), *const ws = (char *)(uintptr_t)(1 << 24);
    for (const Call &c : table) {
        const int n = c.ns + c.nc;
        mpc_lqr_problem p;
        memset(&p, 0, sizeof(p));
        p.B = c.B; p.T = c.T; p.ns = c.ns; p.nc = c.nc; p.dtype = MPC_F32;
        p.x_init = p.C = p.c = p.F = p.f = p.cur_x = p.cur_u = ptr;
        p.C_st = (int64_t)c.B * n * n; p.C_sb = n * n; p.c_st = c.B * n; p.c_sb = n;
        p.F_st = (int64_t)c.B * c.ns * n; p.F_sb = c.ns * n; p.f_st = c.B * c.ns; p.f_sb = c.ns;
        mpc_lqr_options o;
        memset(&o, 0, sizeof(o));
        o.bound_mode = c.bounds; o.lo_s = -1; o.hi_s = 1; o.max_linesearch_iter = 10; o.linesearch_decay = 0.2; o.delta_u = 0.0 / 0.0; o.pnqp_iter = 20;
        mpc_env_dynamics env;
        memset(&env, 0, sizeof(env));
        env.kind = c.sim; env.linearize = c.linearize; env.params = ptr; env.dt = 0.05; env.u_max = 2.0;
        if (c.sim) o.true_dynamics = &env;
        mpc_lqr_outputs out;
        memset(&out, 0, sizeof(out));
        out.new_x = out.new_u = out.costs = out.old_costs = out.full_du_norm = out.alpha_du_norm = out.alphas = ptr;
        out.qp_iters = out.status = (int32_t *)ptr;
        const int64_t bytes = mpc_lqr_workspace_bytes(&p);
        int ring = 0, kernel = 0;
        std::vector<double> ns_per_call;
        for (int r = 0; r < repeats + 1; ++r) {              // (the first repeat warms up and is dropped)
            const auto t0 = std::chrono::steady_clock::now();
            for (long i = 0; i < calls; ++i) kernel += mpc_lqr_step_route(&p, &o, &out, ws, bytes, 0, &ring);
            const double dt = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
            if (r) ns_per_call.push_back(dt / calls);
        }
        std::sort(ns_per_call.begin(), ns_per_call.end());
        printf("%-14s kernel %d ring %d: median %.1f ns (min %.1f, max %.1f) of %d x %ld calls\n", c.name, (int)(kernel / (calls * (repeats + 1))), ring,
               ns_per_call[repeats / 2], ns_per_call.front(), ns_per_call.back(), repeats, calls);
    }
    return 0;
}
