// TEST INFRASTRUCTURE (not product): csrc/nn_dynamics64.h -- the statements of the float64 NNDynamics kernels -- run on the host.
// The "wavefront" is sixty-four threads around a barrier: lane() is the thread's number, sync() the barrier, xor_get() an exchange
// through a slot per lane.  tests/test_nn_f64_host.py loads this file as a shared library and holds its results to
// oracle/env_oracle.py; with -DNN64_HOST_MAIN it is a stand-alone program (its own main, a small fixed problem checked against a
// scalar restatement below) that the same test builds with the host sanitizers and runs.
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>

#include "nn_dynamics64.h"

using namespace mpclqr;

namespace {

struct HostWave {
    pthread_barrier_t bar;
    double slot[2][64];
    HostWave() { pthread_barrier_init(&bar, nullptr, 64); }
    ~HostWave() { pthread_barrier_destroy(&bar); }
};

struct HostExec {
    HostWave *w;
    int id, phase;
    int lane() const { return id; }
    void sync() { pthread_barrier_wait(&w->bar); }
    // two slot sets in turn: a lane that writes set p again has passed the barrier of the call in between, which every reader of
    // the earlier contents of p reached only after its read
    double xor_get(double v, int mask)
    {
        double *s = w->slot[phase];
        phase ^= 1;
        s[id] = v;
        pthread_barrier_wait(&w->bar);
        return s[id ^ mask];
    }
};

template <typename F> void run_wave(F &&body)
{
    HostWave w;
    std::vector<std::thread> th;
    for (int id = 0; id < 64; ++id)
        th.emplace_back([&w, id, &body]() {
            HostExec ex = {&w, id, 0};
            body(ex);
        });
    for (auto &t : th) t.join();
}

nn64::Net make_net(int L, int act, int pass, int carry, const int *widths, const double *const *W, const double *const *b)
{
    nn64::Net m;
    memset(&m, 0, sizeof m);
    m.L = L; m.act = act; m.pass = pass; m.carry = carry;
    for (int l = 0; l <= L; ++l) m.w[l] = widths[l];
    for (int l = 0; l < L; ++l) m.W[l] = W[l], m.b[l] = b[l];
    nn64::net_layout(m);
    return m;
}

}  // namespace

extern "C" {

// dense [T,B,n,n] / [T,B,n] costs (C may be NULL: no cost), gains K [T,B,nc,ns] / k (NULL: util.get_traj); delta_u < 0: none
int nn64_host_rollout(int B, int T, int ns, int nc, const double *x_init, const double *C, const double *c, const double *cur_x,
                      const double *cur_u, const double *K, const double *k, const double *old_costs, int bound_mode, double lo_s,
                      double hi_s, const double *lo, const double *hi, const uint8_t *zero_mask, double delta_u, double decay, int max_ls,
                      int L, int act, int pass, int carry, const int *widths, const double *const *W, const double *const *b, int staged,
                      double *new_x, double *new_u, double *costs, double *full_du_norm, double *alpha_du_norm, double *alphas,
                      int32_t *status)
{
    const nn64::Net m = make_net(L, act, pass, carry, widths, W, b);
    const int n = ns + nc;
    StepParams<double> p;
    memset(&p, 0, sizeof p);
    p.B = B; p.T = T; p.ns = ns; p.nc = nc;
    p.x_init = x_init; p.C = C; p.c = c; p.cur_x = cur_x; p.cur_u = cur_u;
    p.C_st = (long)B * n * n; p.C_sb = (long)n * n; p.c_st = (long)B * n; p.c_sb = n;
    p.bound_mode = bound_mode; p.lo_s = lo_s; p.hi_s = hi_s; p.lo = lo; p.hi = hi; p.zero_mask = zero_mask;
    p.has_delta = delta_u >= 0; p.delta_u = p.has_delta ? delta_u : 0.0;
    p.ls_decay = decay; p.max_ls = max_ls;
    p.K = const_cast<double *>(K); p.k = const_cast<double *>(k); p.old_costs_in = old_costs;
    p.new_x = new_x; p.new_u = new_u; p.costs = costs; p.full_du_norm = full_du_norm; p.alpha_du_norm = alpha_du_norm;
    p.alphas = alphas; p.status = status;
    // exactly the doubles the launch plan gives a wavefront (+ the staged network): an index past them is a heap overflow here
    std::vector<double> lds((staged ? m.total : 0) + nn64::rollout_wave_doubles(m));
    double *base = lds.data(), *area = base + (staged ? m.total : 0);
    run_wave([&](HostExec &ex) {
        if (staged) {
            nn64::stage_net(m, base, ex.lane(), 64);
            ex.sync();
        }
        for (long bi = 0; bi < B; ++bi) {
            if (staged) nn64::rollout_problem<true>(ex, p, m, base, area, bi);
            else nn64::rollout_problem<false>(ex, p, m, base, area, bi);
            ex.sync();
        }
    });
    return 0;
}

int nn64_host_linearize(long N, int ns, int nc, const double *x, const double *u, int L, int act, int pass, const int *widths,
                        const double *const *W, const double *const *b, int staged, double *F, double *f)
{
    const nn64::Net m = make_net(L, act, pass, 0, widths, W, b);
    const int n = ns + nc;
    std::vector<double> lds((staged ? m.total : 0) + nn64::linearize_wave_doubles(m));
    double *base = lds.data(), *area = base + (staged ? m.total : 0);
    run_wave([&](HostExec &ex) {
        if (staged) {
            nn64::stage_net(m, base, ex.lane(), 64);
            ex.sync();
        }
        for (long i = 0; i < N; ++i) {
            if (staged) nn64::linearize_point<true>(ex, m, base, area, ns, nc, x + i * ns, u + i * nc, F + i * ns * n, f + i * ns);
            else nn64::linearize_point<false>(ex, m, base, area, ns, nc, x + i * ns, u + i * nc, F + i * ns * n, f + i * ns);
        }
    });
    return 0;
}

}  // extern "C"

#ifdef NN64_HOST_MAIN
// A (5, 2, [7, 6, 9]) elu network with passthrough and a (3, 1, []) bare layer: trajectory, line-searched rollout under a box and
// the linearisation, staged and in place, against a scalar restatement (forward by loops, Jacobian by central differences).
namespace {

double rnd(unsigned &s) { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 32768.0 - 1.0; }

struct TestNet {
    int L, act, pass, widths[5];
    std::vector<std::vector<double>> W, b;
    std::vector<const double *> Wp, bp;
};

TestNet make(int ns, int nc, std::vector<int> hidden, int act, int pass, unsigned seed)
{
    TestNet t;
    t.L = (int)hidden.size() + 1; t.act = act; t.pass = pass;
    t.widths[0] = ns + nc;
    for (size_t i = 0; i < hidden.size(); ++i) t.widths[i + 1] = hidden[i];
    t.widths[t.L] = ns;
    for (int l = 0; l < t.L; ++l) {
        t.W.emplace_back((size_t)t.widths[l] * t.widths[l + 1]);
        t.b.emplace_back(t.widths[l + 1]);
        for (auto &v : t.W.back()) v = 0.6 * rnd(seed);
        for (auto &v : t.b.back()) v = 0.3 * rnd(seed);
    }
    for (int l = 0; l < t.L; ++l) t.Wp.push_back(t.W[l].data()), t.bp.push_back(t.b[l].data());
    return t;
}

void forward(const TestNet &t, const double *tau, int ns, double *out)
{
    std::vector<double> a(tau, tau + t.widths[0]), z;
    for (int l = 0; l < t.L; ++l) {
        z.assign(t.widths[l + 1], 0.0);
        for (int o = 0; o < t.widths[l + 1]; ++o) {
            double s = t.b[l][o];
            for (int j = 0; j < t.widths[l]; ++j) s += t.W[l][(size_t)o * t.widths[l] + j] * a[j];
            z[o] = l + 1 < t.L ? nn64::act_fn(s, t.act) : s;
        }
        a = z;
    }
    for (int i = 0; i < ns; ++i) out[i] = a[i] + (t.pass ? tau[i] : 0.0);
}

int check(const char *what, double got, double want, double tol)
{
    if (fabs(got - want) <= tol * (1.0 + fabs(want))) return 0;
    printf("MISMATCH %s: %.17g against %.17g\n", what, got, want);
    return 1;
}

int run_case(int ns, int nc, std::vector<int> hidden, int act, int pass, int staged)
{
    const int B = 3, T = 5, n = ns + nc;
    unsigned seed = 12345u + ns;
    TestNet t = make(ns, nc, hidden, act, pass, seed);
    std::vector<double> x0(B * ns), u((size_t)T * B * nc), C((size_t)T * B * n * n, 0.0), c((size_t)T * B * n), K((size_t)T * B * nc * ns),
        k((size_t)T * B * nc);
    for (auto &v : x0) v = rnd(seed);
    for (auto &v : u) v = 0.3 * rnd(seed);
    for (auto &v : c) v = rnd(seed);
    for (auto &v : K) v = 0.2 * rnd(seed);
    for (auto &v : k) v = 0.5 * rnd(seed);
    for (size_t tb = 0; tb < (size_t)T * B; ++tb)
        for (int i = 0; i < n; ++i) C[(tb * n + i) * n + i] = 1.0 + 0.1 * i;
    int bad = 0;
    // trajectory and its cost
    std::vector<double> xs((size_t)T * B * ns), cost(B), ref(ns);
    nn64_host_rollout(B, T, ns, nc, x0.data(), C.data(), c.data(), nullptr, u.data(), nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr,
                      nullptr, -1.0, 0.2, 1, t.L, t.act, t.pass, 0, t.widths, t.Wp.data(), t.bp.data(), staged, xs.data(), nullptr,
                      cost.data(), nullptr, nullptr, nullptr, nullptr);
    for (int bi = 0; bi < B; ++bi) {
        std::vector<double> tau(n);
        double J = 0.0;
        for (int i = 0; i < ns; ++i) tau[i] = x0[bi * ns + i];
        for (int ti = 0; ti < T; ++ti) {
            const size_t tb = (size_t)ti * B + bi;
            for (int i = 0; i < nc; ++i) tau[ns + i] = u[tb * nc + i];
            for (int i = 0; i < ns; ++i) bad += check("traj", xs[tb * ns + i], tau[i], 1e-12);
            for (int i = 0; i < n; ++i) J += 0.5 * C[(tb * n + i) * n + i] * tau[i] * tau[i] + c[tb * n + i] * tau[i];
            forward(t, tau.data(), ns, ref.data());
            for (int i = 0; i < ns; ++i) tau[i] = ref[i];
        }
        bad += check("cost", cost[bi], J, 1e-12);
    }
    // the line-searched rollout: every accepted trajectory obeys the network, the box and the control law
    std::vector<double> nx((size_t)T * B * ns), nu((size_t)T * B * nc), nc_(B), full(B), adu(B), al(B);
    std::vector<int32_t> st(B, 0);
    nn64_host_rollout(B, T, ns, nc, x0.data(), C.data(), c.data(), xs.data(), u.data(), K.data(), k.data(), cost.data(), 1, -0.4, 0.4,
                      nullptr, nullptr, nullptr, -1.0, 0.2, 4, t.L, t.act, t.pass, 0, t.widths, t.Wp.data(), t.bp.data(), staged, nx.data(),
                      nu.data(), nc_.data(), full.data(), adu.data(), al.data(), st.data());
    for (int bi = 0; bi < B; ++bi) {
        std::vector<double> tau(n);
        double J = 0.0;
        for (int ti = 0; ti < T; ++ti) {
            const size_t tb = (size_t)ti * B + bi;
            for (int i = 0; i < ns; ++i) tau[i] = nx[tb * ns + i];
            for (int i = 0; i < nc; ++i) {
                double v = u[tb * nc + i] + al[bi] * k[tb * nc + i];
                for (int j = 0; j < ns && ti > 0; ++j) v += K[(tb * nc + i) * ns + j] * (tau[j] - xs[tb * ns + j]);
                v = v < -0.4 ? -0.4 : (v > 0.4 ? 0.4 : v);
                bad += check("new_u", nu[tb * nc + i], v, 1e-12);
                tau[ns + i] = nu[tb * nc + i];
            }
            for (int i = 0; i < n; ++i) J += 0.5 * C[(tb * n + i) * n + i] * tau[i] * tau[i] + c[tb * n + i] * tau[i];
            if (ti + 1 < T) {
                forward(t, tau.data(), ns, ref.data());
                for (int i = 0; i < ns; ++i) bad += check("new_x", nx[(tb + B) * ns + i], ref[i], 1e-12);
            }
        }
        bad += check("costs", nc_[bi], J, 1e-11);
        if (!(al[bi] == 1.0 || nc_[bi] <= cost[bi] || al[bi] < 0.009)) bad += printf("MISMATCH line search of problem %d\n", bi);
    }
    // the linearisation against central differences
    const long N = (long)(T - 1) * B;
    std::vector<double> F((size_t)N * ns * n), f((size_t)N * ns), hi(ns), lo(ns);
    nn64_host_linearize(N, ns, nc, xs.data(), u.data(), t.L, t.act, t.pass, t.widths, t.Wp.data(), t.bp.data(), staged, F.data(), f.data());
    for (long i = 0; i < N; ++i) {
        std::vector<double> tau(n);
        for (int j = 0; j < ns; ++j) tau[j] = xs[i * ns + j];
        for (int j = 0; j < nc; ++j) tau[ns + j] = u[i * nc + j];
        forward(t, tau.data(), ns, ref.data());
        for (int r = 0; r < ns; ++r) {
            double Ft = 0.0;
            for (int j = 0; j < n; ++j) Ft += F[(i * ns + r) * n + j] * tau[j];
            bad += check("f", f[i * ns + r], ref[r] - Ft, 1e-11);
        }
        for (int j = 0; j < n; ++j) {
            std::vector<double> tp(tau), tm(tau);
            tp[j] += 1e-6; tm[j] -= 1e-6;
            forward(t, tp.data(), ns, hi.data());
            forward(t, tm.data(), ns, lo.data());
            for (int r = 0; r < ns; ++r) bad += check("F", F[(i * ns + r) * n + j], (hi[r] - lo[r]) / 2e-6, 1e-7);
        }
    }
    return bad;
}

}  // namespace

int main()
{
    int bad = 0;
    for (int staged = 0; staged < 2; ++staged) {
        bad += run_case(5, 2, {7, 6, 9}, MPC_ACT_ELU, 1, staged);
        bad += run_case(3, 1, {}, MPC_ACT_SIGMOID, 0, staged);
        bad += run_case(4, 3, {70}, MPC_ACT_SIGMOID, 1, staged);
    }
    printf(bad ? "nn64_host: %d mismatches\n" : "nn64_host: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
