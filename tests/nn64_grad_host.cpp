// TEST INFRASTRUCTURE (not product): csrc/nn_param_grad64.h -- the statements of the float64 NNDynamics weight-gradient kernels -- run
// on the host.  The "block" is PG64_THREADS threads around a barrier: tid() is the thread's number, sync() the barrier; a thread's
// wavefront is the sixty-four threads tid() >> 6, which exchange through a slot per lane behind a barrier of their own (xor_get()).
// The LDS stand-in is a heap block of exactly the doubles the launch plan gives a block, the blocks of the grid run one after the
// other.  tests/test_nn_f64_grad_host.py loads this file as a shared library and holds its results to the float64 yardstick; with
// -DNN64_GRAD_HOST_MAIN it is a stand-alone program (its own main: small fixed problems checked against central differences of a
// scalar restatement) that the same test builds with the host sanitizers and runs.
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>

#include "nn_param_grad64.h"

using namespace mpclqr;

namespace {

constexpr int NT = nn64::PG64_THREADS, NW = NT / 64;

struct HostBlock {
    pthread_barrier_t bar, wbar[NW];
    double slot[NW][2][64];
    HostBlock()
    {
        pthread_barrier_init(&bar, nullptr, NT);
        for (auto &w : wbar) pthread_barrier_init(&w, nullptr, 64);
    }
    ~HostBlock()
    {
        pthread_barrier_destroy(&bar);
        for (auto &w : wbar) pthread_barrier_destroy(&w);
    }
};

struct HostExec {
    HostBlock *blk;
    int id, phase;
    int lane() const { return id & 63; }
    int tid() const { return id; }
    void sync() { pthread_barrier_wait(&blk->bar); }
    // two slot sets in turn (tests/nn64_host.cpp): a lane that writes set p again has passed the barrier of the call in between
    double xor_get(double v, int mask)
    {
        const int w = id >> 6;
        double *s = blk->slot[w][phase];
        phase ^= 1;
        s[id & 63] = v;
        pthread_barrier_wait(&blk->wbar[w]);
        return s[(id & 63) ^ mask];
    }
};

nn64::Net make_net(int L, int act, int pass, const int *widths, const double *const *W, const double *const *b)
{
    nn64::Net m;
    memset(&m, 0, sizeof m);
    m.L = L; m.act = act; m.pass = pass; m.carry = 0;
    for (int l = 0; l <= L; ++l) m.w[l] = widths[l];
    for (int l = 0; l < L; ++l) m.W[l] = W[l], m.b[l] = b[l];
    nn64::net_layout(m);
    return m;
}

template <bool WL, int KMAX>
void run_grid(const nn64::Net &m, const nn64::GradLayout &g, long N, int blocks, int ns, int nc, const double *x, const double *u,
              const double *gF, const double *gf, double *partials)
{
    const long n = ns + nc;
    // exactly the doubles the launch plan gives a block (+ the staged network): an index past them is a heap overflow here
    std::vector<double> lds((WL ? m.total : 0) + g.doubles);
    double *base = lds.data(), *area = base + (WL ? m.total : 0);
    for (int blk = 0; blk < blocks; ++blk) {
        HostBlock hb;
        std::vector<std::thread> th;
        for (int id = 0; id < NT; ++id)
            th.emplace_back([&, id]() {
                HostExec ex = {&hb, id, 0};
                if (WL) {
                    nn64::stage_net(m, base, id, NT);
                    ex.sync();
                }
                double acc[KMAX];
                for (int k = 0; k < KMAX; ++k) acc[k] = 0.0;
                for (long i = blk; i < N; i += blocks)
                    nn64::param_grad_point<WL, KMAX>(ex, m, g, base, area, x + i * ns, u + i * nc, gF + i * ns * n, gf + i * ns, acc);
                double *out = partials + (long)blk * KMAX * NT;
                for (int k = 0; k < KMAX; ++k) out[k * NT + id] = acc[k];
            });
        for (auto &t : th) t.join();
    }
}

}  // namespace

extern "C" {

// what the launch plan gives this network: the KMAX instantiation (0: none), the block's area in doubles, the staged network's doubles
int nn64_grad_host_plan(int L, const int *widths, long *area_doubles, long *staged_doubles)
{
    const double *none[MPC_MLP_MAX_LAYERS] = {};
    const nn64::Net m = make_net(L, 0, 0, widths, none, none);
    const nn64::GradLayout g = nn64::grad_layout(m);
    if (area_doubles) *area_doubles = g.doubles;
    if (staged_doubles) *staged_doubles = m.total;
    return nn64::grad_kmax(g.entries);
}

// `blocks` blocks over N points; partials: blocks * KMAX * PG64_THREADS doubles; gW / gb: L pointers each.  Returns KMAX, -1: no
// instantiation owns the network
int nn64_grad_host(long N, int blocks, int ns, int nc, const double *x, const double *u, const double *gF, const double *gf, int L, int act,
                   int pass, const int *widths, const double *const *W, const double *const *b, int staged, double *partials,
                   double *const *gW, double *const *gb)
{
    const nn64::Net m = make_net(L, act, pass, widths, W, b);
    const nn64::GradLayout g = nn64::grad_layout(m);
    const int kmax = nn64::grad_kmax(g.entries);
    if (!kmax) return -1;
#define RUN(WL, K) run_grid<WL, K>(m, g, N, blocks, ns, nc, x, u, gF, gf, partials)
    if (kmax == nn64::PG64_KMAX_SMALL) staged ? RUN(true, nn64::PG64_KMAX_SMALL) : RUN(false, nn64::PG64_KMAX_SMALL);
    else if (kmax == nn64::PG64_KMAX_MID) staged ? RUN(true, nn64::PG64_KMAX_MID) : RUN(false, nn64::PG64_KMAX_MID);
    else staged ? RUN(true, nn64::PG64_KMAX_LARGE) : RUN(false, nn64::PG64_KMAX_LARGE);
#undef RUN
    nn64::GradFinal a;
    memset(&a, 0, sizeof a);
    a.L = L; a.blocks = blocks; a.stride = (long)kmax * NT; a.partials = partials;
    for (int l = 0; l <= L; ++l) a.w[l] = widths[l];
    for (int l = 0; l < L; ++l) a.gW[l] = gW[l], a.gb[l] = gb[l];
    for (long e = 0; e < g.entries; ++e) nn64::sum_partials(a, e);
    return kmax;
}

}  // extern "C"

#ifdef NN64_GRAD_HOST_MAIN
// Small networks, staged and in place, two blocks over three points, outputs and workspace filled with NaN beforehand: every
// weight's and bias's gradient against a central difference of J = sum_points (gF . F + gf . f), F and f by scalar loops.
namespace {

double rnd(unsigned &s) { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 32768.0 - 1.0; }

struct TestNet {
    int L, act, widths[5];
    std::vector<std::vector<double>> W, b;
};

// J at one point: F = W_L diag(s_{L-1}) W_{L-1} ... diag(s_1) W_1, f = net(tau) - F tau (the passthrough's identity cancels in
// the weights' gradient: left out on both sides)
double objective(const TestNet &t, const double *tau, const double *gF, const double *gf)
{
    const int n = t.widths[0], ns = t.widths[t.L];
    std::vector<double> a(tau, tau + n), z, P((size_t)n * n, 0.0), Q;
    for (int i = 0; i < n; ++i) P[(size_t)i * n + i] = 1.0;
    for (int l = 0; l < t.L; ++l) {
        const int wi = t.widths[l], wo = t.widths[l + 1];
        z.assign(wo, 0.0);
        Q.assign((size_t)wo * n, 0.0);
        for (int o = 0; o < wo; ++o) {
            double s = t.b[l][o];
            for (int j = 0; j < wi; ++j) s += t.W[l][(size_t)o * wi + j] * a[j];
            const bool hidden = l + 1 < t.L;
            z[o] = hidden ? nn64::act_fn(s, t.act) : s;
            const double sl = hidden ? nn64::slope_fn(z[o], t.act) : 1.0;
            for (int c = 0; c < n; ++c) {
                double q = 0.0;
                for (int j = 0; j < wi; ++j) q += t.W[l][(size_t)o * wi + j] * P[(size_t)j * n + c];
                Q[(size_t)o * n + c] = sl * q;
            }
        }
        a = z;
        P = Q;
    }
    double J = 0.0;
    for (int i = 0; i < ns; ++i) {
        double Ft = 0.0;
        for (int c = 0; c < n; ++c) {
            J += gF[(size_t)i * n + c] * P[(size_t)i * n + c];
            Ft += P[(size_t)i * n + c] * tau[c];
        }
        J += gf[i] * (a[i] - Ft);
    }
    return J;
}

int run_case(int ns, int nc, std::vector<int> hidden, int act, int staged)
{
    const int N = 3, blocks = 2, n = ns + nc;
    unsigned seed = 777u + 13 * ns + (unsigned)hidden.size();
    TestNet t;
    t.L = (int)hidden.size() + 1; t.act = act;
    t.widths[0] = n;
    for (size_t i = 0; i < hidden.size(); ++i) t.widths[i + 1] = hidden[i];
    t.widths[t.L] = ns;
    for (int l = 0; l < t.L; ++l) {
        t.W.emplace_back((size_t)t.widths[l] * t.widths[l + 1]);
        t.b.emplace_back(t.widths[l + 1]);
        for (auto &v : t.W.back()) v = 0.8 * rnd(seed);
        for (auto &v : t.b.back()) v = 0.3 * rnd(seed) + 0.05;
    }
    std::vector<double> x((size_t)N * ns), u((size_t)N * nc), gF((size_t)N * ns * n), gf((size_t)N * ns);
    for (auto &v : x) v = rnd(seed);
    for (auto &v : u) v = rnd(seed);
    for (auto &v : gF) v = rnd(seed);
    for (auto &v : gf) v = rnd(seed);
    const int kmax = nn64_grad_host_plan(t.L, t.widths, nullptr, nullptr);
    const double nan = strtod("nan", nullptr);
    std::vector<double> partials((size_t)blocks * kmax * NT, nan);
    std::vector<std::vector<double>> gW, gb;
    std::vector<const double *> Wp, bp;
    std::vector<double *> gWp, gbp;
    for (int l = 0; l < t.L; ++l) {
        gW.emplace_back(t.W[l].size(), nan);
        gb.emplace_back(t.b[l].size(), nan);
    }
    for (int l = 0; l < t.L; ++l) Wp.push_back(t.W[l].data()), bp.push_back(t.b[l].data()), gWp.push_back(gW[l].data()), gbp.push_back(gb[l].data());
    if (nn64_grad_host(N, blocks, ns, nc, x.data(), u.data(), gF.data(), gf.data(), t.L, act, 1, t.widths, Wp.data(), bp.data(), staged,
                       partials.data(), gWp.data(), gbp.data()) != kmax)
        return 1;
    auto J = [&]() {
        double s = 0.0;
        std::vector<double> tau(n);
        for (int i = 0; i < N; ++i) {
            for (int j = 0; j < n; ++j) tau[j] = j < ns ? x[(size_t)i * ns + j] : u[(size_t)i * nc + j - ns];
            s += objective(t, tau.data(), gF.data() + (size_t)i * ns * n, gf.data() + (size_t)i * ns);
        }
        return s;
    };
    int bad = 0;
    const double h = 1e-6;
    for (int l = 0; l < t.L; ++l)
        for (int which = 0; which < 2; ++which) {
            std::vector<double> &p = which ? t.b[l] : t.W[l];
            const std::vector<double> &got = which ? gb[l] : gW[l];
            for (size_t e = 0; e < p.size(); ++e) {
                const double keep = p[e];
                p[e] = keep + h;
                const double hi = J();
                p[e] = keep - h;
                const double lo = J();
                p[e] = keep;
                const double want = (hi - lo) / (2 * h);
                if (!(fabs(got[e] - want) <= 1e-6 * (1.0 + fabs(want)))) {
                    printf("MISMATCH layer %d %s[%zu]: %.17g against %.17g\n", l + 1, which ? "b" : "W", e, got[e], want);
                    ++bad;
                }
            }
        }
    return bad;
}

}  // namespace

int main()
{
    int bad = 0;
    for (int staged = 0; staged < 2; ++staged) {
        bad += run_case(3, 1, {}, MPC_ACT_SIGMOID, staged);
        bad += run_case(4, 2, {9}, MPC_ACT_SIGMOID, staged);
        bad += run_case(3, 2, {7, 6}, MPC_ACT_RELU, staged);
        bad += run_case(3, 1, {5, 6, 4}, MPC_ACT_SIGMOID, staged);
    }
    printf(bad ? "nn64_grad_host: %d mismatches\n" : "nn64_grad_host: ok\n", bad);
    return bad ? 1 : 0;
}
#endif
