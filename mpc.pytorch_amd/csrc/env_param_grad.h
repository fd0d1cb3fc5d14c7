// env_param_grad.h -- the backward half of the simulator linearisation (env_dynamics.h): for one trajectory point,
// the gradient of  sum(gF * F) + sum(gf * f)  with respect to the simulator's parameters, where
//     F = d env(x,u) / d [x;u],   f = env(x,u) - F [x;u]     (MPC.linearize_dynamics, mpc/mpc.py:490-549)
// and x, u are constants (the linearisation works on detached leaves, :495-497):
//
//     g_k = sum_r gf_r d out_r / d p_k  +  sum_{r,j} (gF_rj - gf_r tau_j) d J_rj / d p_k ,     tau = [x; u].
//
// The derivatives are not written down a second time: env_step itself is instantiated on a number type that carries
// one tangent per parameter, so d out / d p and d J / d p are whatever the transition and the Jacobian every rollout
// kernel runs differentiate to -- the two cannot drift apart.  The primal part of every operation is the very
// function env_step calls for plain numbers (env_inv, env_rsqrt, env_sincos with its float32 fast-trig range test),
// the clamp and range selects are selects of whole (value, tangent) pairs: outside the clamp the control column of J
// is the constant 0 and so is its parameter derivative, on the closed interval the clamp's derivative is 1.
// Compiles for the host with a plain C++ compiler, like env_dynamics.h.
#pragma once
#include <type_traits>
#include "env_dynamics.h"

namespace mpclqr {

template <typename T, int NP> struct EnvDual {
    T v;          // value
    T d[NP];      // d value / d p_k
    EnvDual() = default;
    template <typename S, typename = typename std::enable_if<std::is_arithmetic<S>::value>::type>
    MPC_HD EnvDual(S s) : v((T)s)
    {
#pragma unroll
        for (int k = 0; k < NP; ++k) d[k] = 0;
    }
    MPC_HD friend EnvDual operator-(const EnvDual &a)
    {
        EnvDual r;
        r.v = -a.v;
#pragma unroll
        for (int k = 0; k < NP; ++k) r.d[k] = -a.d[k];
        return r;
    }
    MPC_HD friend EnvDual operator+(const EnvDual &a, const EnvDual &b)
    {
        EnvDual r;
        r.v = a.v + b.v;
#pragma unroll
        for (int k = 0; k < NP; ++k) r.d[k] = a.d[k] + b.d[k];
        return r;
    }
    MPC_HD friend EnvDual operator-(const EnvDual &a, const EnvDual &b)
    {
        EnvDual r;
        r.v = a.v - b.v;
#pragma unroll
        for (int k = 0; k < NP; ++k) r.d[k] = a.d[k] - b.d[k];
        return r;
    }
    MPC_HD friend EnvDual operator*(const EnvDual &a, const EnvDual &b)
    {
        EnvDual r;
        r.v = a.v * b.v;
#pragma unroll
        for (int k = 0; k < NP; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
        return r;
    }
    // comparisons look at the value alone (which side of a clamp / range test a point is on does not move with p)
    MPC_HD friend bool operator<(const EnvDual &a, const EnvDual &b) { return a.v < b.v; }
    MPC_HD friend bool operator>(const EnvDual &a, const EnvDual &b) { return a.v > b.v; }
    MPC_HD friend bool operator<=(const EnvDual &a, const EnvDual &b) { return a.v <= b.v; }
    MPC_HD friend bool operator>=(const EnvDual &a, const EnvDual &b) { return a.v >= b.v; }
};

// env_step on these numbers is always asked for its Jacobian (env_dynamics.h)
template <typename T, int NP> MPC_HD bool env_wants_jacobian(const EnvDual<T, NP> *) { return true; }

// value through env_step's own helper, tangent by the chain rule on that value
template <typename T, int NP> MPC_HD EnvDual<T, NP> env_inv(const EnvDual<T, NP> &a)
{
    EnvDual<T, NP> r;
    r.v = env_inv(a.v);
    const T m = -r.v * r.v;
#pragma unroll
    for (int k = 0; k < NP; ++k) r.d[k] = m * a.d[k];
    return r;
}
template <typename T, int NP> MPC_HD EnvDual<T, NP> env_rsqrt(const EnvDual<T, NP> &a)
{
    EnvDual<T, NP> r;
    r.v = env_rsqrt(a.v);
    const T m = (T)-0.5 * r.v * r.v * r.v;
#pragma unroll
    for (int k = 0; k < NP; ++k) r.d[k] = m * a.d[k];
    return r;
}
template <typename T, int NP> MPC_HD void env_sincos(const EnvDual<T, NP> &a, EnvDual<T, NP> &s, EnvDual<T, NP> &c)
{
    env_sincos(a.v, s.v, c.v);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        s.d[k] = c.v * a.d[k];
        c.d[k] = -s.v * a.d[k];
    }
}
template <typename T, int NP> MPC_HD EnvDual<T, NP> env_sin(const EnvDual<T, NP> &a)
{
    EnvDual<T, NP> r;
    T s, c;
    env_sincos(a.v, s, c);          // (the same range test as env_sin / env_cos: one for both)
    r.v = s;
#pragma unroll
    for (int k = 0; k < NP; ++k) r.d[k] = c * a.d[k];
    return r;
}
template <typename T, int NP> MPC_HD EnvDual<T, NP> env_cos(const EnvDual<T, NP> &a)
{
    EnvDual<T, NP> r;
    T s, c;
    env_sincos(a.v, s, c);
    r.v = c;
#pragma unroll
    for (int k = 0; k < NP; ++k) r.d[k] = -s * a.d[k];
    return r;
}
template <typename T, int NP> MPC_HD EnvDual<T, NP> atan2(const EnvDual<T, NP> &y, const EnvDual<T, NP> &x)
{
    EnvDual<T, NP> r;
    r.v = ::atan2(y.v, x.v);
    const T ir2 = env_inv(x.v * x.v + y.v * y.v);
#pragma unroll
    for (int k = 0; k < NP; ++k) r.d[k] = (x.v * y.d[k] - y.v * x.d[k]) * ir2;
    return r;
}

template <int KIND> struct EnvKind {
    static constexpr int ns = KIND == MPC_ENV_CARTPOLE ? 5 : 3;
    static constexpr int np = KIND == MPC_ENV_PENDULUM ? 3 : (KIND == MPC_ENV_PENDULUM_FULL ? 5 : 4);
};

// g[np] for one point.  e.params: the np parameters (plain numbers); gF row-major [ns][ns+1], gf [ns].
template <typename real, int KIND>
MPC_HD void env_param_vjp(const EnvDesc<real> &e, const real *x, real u, const real *gF, const real *gf, real *g)
{
    constexpr int ns = EnvKind<KIND>::ns, np = EnvKind<KIND>::np, n = ns + 1;
    typedef EnvDual<real, np> D;
    D prm[np], xd[ns], out[ns], J[ns * n];
#pragma unroll
    for (int k = 0; k < np; ++k) {
        prm[k] = D(e.params[k]);
        prm[k].d[k] = 1;
    }
#pragma unroll
    for (int j = 0; j < ns; ++j) xd[j] = D(x[j]);
    EnvDesc<D> ed;
    ed.kind = KIND;
    ed.linearize = 0;
    ed.params = prm;
    ed.dt = D(e.dt);
    ed.u_max = D(e.u_max);
    env_step<D>(ed, xd, D(u), out, J);
#pragma unroll
    for (int k = 0; k < np; ++k) g[k] = 0;
#pragma unroll
    for (int r = 0; r < ns; ++r) {
        const real w = gf[r];
#pragma unroll
        for (int k = 0; k < np; ++k) g[k] += w * out[r].d[k];
#pragma unroll
        for (int j = 0; j < n; ++j) {
            const real coef = gF[r * n + j] - w * (j < ns ? x[j] : u);
#pragma unroll
            for (int k = 0; k < np; ++k) g[k] += coef * J[r * n + j].d[k];
        }
    }
}

// the same by the descriptor's own kind (host callers; the kernels are instantiated per kind)
template <typename real>
MPC_HD void env_param_vjp(const EnvDesc<real> &e, const real *x, real u, const real *gF, const real *gf, real *g)
{
    if (e.kind == MPC_ENV_PENDULUM) env_param_vjp<real, MPC_ENV_PENDULUM>(e, x, u, gF, gf, g);
    else if (e.kind == MPC_ENV_PENDULUM_FULL) env_param_vjp<real, MPC_ENV_PENDULUM_FULL>(e, x, u, gF, gf, g);
    else env_param_vjp<real, MPC_ENV_CARTPOLE>(e, x, u, gF, gf, g);
}

}  // namespace mpclqr
