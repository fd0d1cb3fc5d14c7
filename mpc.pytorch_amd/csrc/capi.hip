// capi.hip -- extern "C" entry points of libmpc_lqr_hip.so (declared in include/mpc_lqr.h).
// Argument validation + dtype / kernel dispatch; no computation happens on the host.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "lqr_common.h"

namespace mpclqr {
static thread_local std::string g_last_error;
void set_last_error(const char *msg) { g_last_error = msg ? msg : ""; }

static int fail(int code, const char *msg)
{
    set_last_error(msg);
    return code;
}

// f(real()) with the `real` of a dtype the caller has checked: the float / double pair of an entry point written once
template <typename F>
static int by_dtype(int dtype, F &&f)
{
    return dtype == MPC_F32 ? f(float()) : f(double());
}

// A two-valued switch of the environment ("2" / "4", "0" / "1": its first character decides), `unset` where it is absent or says
// anything else.
struct EnvSwitch { const char *name; char a, b; int unset; };
static const EnvSwitch SW_DPP16_RING = {"MPC_DPP16_RING", '2', '4', 0};              // A/B switch of the 12/4 kernel's staging ring
static const EnvSwitch SW_MFMA40_RING = {"MPC_MFMA40_RING", '2', '3', 0};            // the 32/8 kernel's sweep ring
static const EnvSwitch SW_DPP16_RESIDENT = {"MPC_DPP16_RESIDENT", '0', '1', -1};     // A/B switch of the resident-F build (see dpp16_resident)
static int read_switch(const EnvSwitch &s)
{
    const char *e = getenv(s.name);
    return (e && (e[0] == s.a || e[0] == s.b)) ? e[0] - '0' : s.unset;
}

// Read once per process (the first launch): the three switches and the number of SIMDs of the device the library runs on (MI355X:
// 256 CUs x 4), which is where the constrained step changes rings.
struct DeviceFacts {
    int ring_force;      // 0 = pick by mode and batch, 2 / 4 = MPC_DPP16_RING
    int simds;
    int ring40_force;    // 0 = pick by mode and batch, 2 / 3 = MPC_MFMA40_RING
    bool sticky;         // false with MPC_DPP16_RING_DYNAMIC set: the switches are re-read at every launch (the tests flip them)
    int resident;        // MPC_DPP16_RESIDENT: 0 / 1, -1 = not set (the default, see dpp16_resident)
};
static const DeviceFacts &device_facts()
{
    static DeviceFacts f = [] {
        DeviceFacts d;
        d.simds = 1024;
        hipDeviceProp_t prop;
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            d.simds = prop.multiProcessorCount * 4;
        d.ring_force = read_switch(SW_DPP16_RING);
        d.ring40_force = read_switch(SW_MFMA40_RING);
        d.sticky = getenv("MPC_DPP16_RING_DYNAMIC") == nullptr;
        d.resident = read_switch(SW_DPP16_RESIDENT);
        return d;
    }();
    return f;
}
// a switch as a launch sees it: what the process read at load, or -- MPC_DPP16_RING_DYNAMIC=1, the test suite -- the environment of
// this very launch
static int env_switch(const EnvSwitch &s, int at_load) { return device_facts().sticky ? at_load : read_switch(s); }

// The mode-0 12/4 step on the two-slot ring with a share of F kept in LDS between sweep and rollout (lqr_dpp16_res.o): 39 KiB a wave,
// so only while one wavefront per SIMD holds the batch -- beyond, 40 KiB would halve the occupancy the short ring is there for.
constexpr bool DPP16_RESIDENT_DEFAULT = true;
static std::atomic<int64_t> g_resident_launches{0};          // mpc_lqr_resident_launches
static bool dpp16_resident(const StepParams<float> &q)
{
    const DeviceFacts &f = device_facts();
    int on = env_switch(SW_DPP16_RESIDENT, f.resident);
    // Unforced, only where the launch is bound by its traffic: the kept blocks cost the wavefront's own chain ~3.5 us (the copy, the choice
    // of base and of DMA source at every timestep), which shows wherever the chain is the launch -- paired, MI355X: B = 2048 +3.6 us,
    // 3072 +3.5, 3584 +1.2, 3840 -0.5, 4096 -1.75 (docs/history/r20.md).  Beyond 15/16 of one wavefront per SIMD it pays.
    const int waves = (q.B + 3) / 4;
    if (on < 0) on = (DPP16_RESIDENT_DEFAULT && 16 * (long)waves > 15 * (long)f.simds) ? 1 : 0;
    return on != 0 && q.bound_mode == MPC_BOUND_NONE && !q.zero_mask && q.T >= 2 && q.T <= 64 /* dpp16::RG_STEPS */ && !q.sweep_only &&
           (q.B + 3) / 4 <= f.simds;
}

// The 32/8 kernel's sweep ring: three slots (the DMA two timesteps ahead: address-translation misses behind another kernel
// stay hidden, lqr_mfma40_body.h) wherever four wavefronts per CU are all the batch asks for or the mode gains from them anyway
// (unconstrained / masked: 2.33 against 2.40 ms at B = 8192); the box-constrained step of a larger batch wants six per CU on
// the two-slot ring (round 3: 4.65 against 5.06 ms; round 4, after the QP's rewrite: 3.05 against 3.11).  MPC_MFMA40_RING=2|3 forces one (read like MPC_DPP16_RING).
static int mfma40_ring(const StepParams<float> &sp)
{
    const DeviceFacts &f = device_facts();
    const int force = env_switch(SW_MFMA40_RING, f.ring40_force);
    if (force) return force;
    // Box-constrained: the three-slot ring while one wave per SIMD holds the batch, six waves per CU on the two-slot ring beyond.
    // Unconstrained / masked (round 4, final kernels, config 5 by HIP events): the two-slot ring keeps 1,536 waves resident, so a
    // batch between 1,025 and 1,536 runs in ONE round on it (B = 1,536: 0.44 against 0.54 ms); beyond, the three-slot ring's
    // shorter rounds win (2,048: 0.57 against 0.72 ms; 4,096: 1.11 against 1.21; 8,192: 2.22 against 2.30).  Up to 1,024 the two-slot
    // ring is 1.4-3 % faster in the sustained state (277 against 281 us) but 30 % SLOWER behind a kernel that emptied the address
    // translations (bench.py's cold_translations row: 0.436 against 0.33 ms) -- what the third slot is there for: it stays.
    if (sp.bound_mode != MPC_BOUND_NONE) return sp.B > f.simds ? 2 : 3;
    return (sp.B > f.simds && sp.B <= f.simds + f.simds / 2) ? 2 : 3;
}

static int check_problem(const mpc_lqr_problem *p, bool need_cost, bool need_nominal, bool need_F = true)
{
    if (!p) return fail(MPC_E_NULL, "problem is NULL");
    if (p->B < 0 || p->T < 1 || p->ns < 1 || p->nc < 1) return fail(MPC_E_DIMS, "need B>=0, T>=1, ns>=1, nc>=1");
    if (p->nc > 64) return fail(MPC_E_DIMS, "n_ctrl > 64 is not supported");
    if (p->dtype != MPC_F32 && p->dtype != MPC_F64) return fail(MPC_E_DTYPE, "dtype must be MPC_F32 or MPC_F64");
    if (p->B == 0) return MPC_OK;
    if (need_cost && (!p->C || !p->c)) return fail(MPC_E_NULL, "C / c is NULL");
    if (need_F && p->T > 1 && !p->F) return fail(MPC_E_NULL, "F is NULL");
    if (!p->x_init) return fail(MPC_E_NULL, "x_init is NULL");
    if (need_nominal && (!p->cur_x || !p->cur_u)) return fail(MPC_E_NULL, "current_x / current_u is NULL");
    return MPC_OK;
}

static int check_env(const mpc_env_dynamics *e, int ns, int nc)
{
    // MPC_ENV_CTRL_CARRY rides in `kind`: the state is (previous control, x), one more than the simulator's own
    const int kind = e->kind & ~MPC_ENV_CTRL_CARRY, carry = (e->kind & MPC_ENV_CTRL_CARRY) ? 1 : 0;
    if (kind < MPC_ENV_PENDULUM || kind > MPC_ENV_CARTPOLE) return fail(MPC_E_ARG, "unknown simulator kind");
    if (!e->params) return fail(MPC_E_NULL, "simulator params is NULL");
    if (nc != 1 || ns != env_ns(kind) + carry) return fail(MPC_E_DIMS, "n_state / n_ctrl do not match the simulator");
    if (!(e->dt > 0) || !(e->u_max >= 0)) return fail(MPC_E_ARG, "simulator dt / u_max");
    return MPC_OK;
}

// the argument checks mpc_env_linearize and mpc_env_param_grad share: the simulator itself at N points
static int check_env_points(const mpc_env_dynamics *env, int dtype, int64_t N)
{
    if (!env) return fail(MPC_E_NULL, "simulator is NULL");
    if (dtype != MPC_F32 && dtype != MPC_F64) return fail(MPC_E_DTYPE, "bad dtype");
    if (env->kind & MPC_ENV_CTRL_CARRY) return fail(MPC_E_UNSUPPORTED, "MPC_ENV_CTRL_CARRY: linearise the simulator itself (the carry block is constant)");
    if (env->kind < MPC_ENV_PENDULUM || env->kind > MPC_ENV_CARTPOLE) return fail(MPC_E_ARG, "unknown simulator kind");
    const int rc = check_env(env, env_ns(env->kind), 1);
    if (rc) return rc;
    return N < 0 ? fail(MPC_E_DIMS, "N < 0") : MPC_OK;
}

static int check_options(const mpc_lqr_problem *p, const mpc_lqr_options *o)
{
    if (!o) return MPC_OK;
    if (o->bound_mode < MPC_BOUND_NONE || o->bound_mode > MPC_BOUND_TENSOR) return fail(MPC_E_ARG, "bad bound_mode");
    if (o->bound_mode == MPC_BOUND_TENSOR && (!o->lo || !o->hi) && p->B > 0) return fail(MPC_E_NULL, "tensor bounds are NULL");
    if (o->max_linesearch_iter < 1) return fail(MPC_E_ARG, "max_linesearch_iter must be > 0");  // mpc/mpc.py:148
    // mpc/lqr_step.py:195: delta_u without bounds is unimplemented in the reference as well
    if (o->delta_u == o->delta_u && o->delta_u >= 0 && o->bound_mode == MPC_BOUND_NONE)
        return fail(MPC_E_ARG, "delta_u requires u_lower/u_upper (mpc/lqr_step.py:195)");
    if (o->true_dynamics) {
        int rc = check_env(o->true_dynamics, p->ns, p->nc);
        if (rc) return rc;
    }
    return MPC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The kernels behind mpc_lqr_step (MPC_IMPL_*, lqr_common.h): what each one takes, what it keeps in the workspace, and -- step_route
// -- which of them takes a call.  mpc_lqr_step, mpc_lqr_step_route, mpc_lqr_impl_supported, mpc_lqr_qp_record and
// mpc_lqr_workspace_bytes all ask here; nothing else in this file spells out a kernel's shape or a record's size.
// ---------------------------------------------------------------------------------------------------------------------

// the sizes of a call and its simulator kind, nothing else: default options, no tensors (so every block counts as aligned)
static mpc_lqr_problem sizes_only(int B, int T, int ns, int nc, int dtype)
{
    mpc_lqr_problem q;
    memset(&q, 0, sizeof(q));
    q.B = B; q.T = T; q.ns = ns; q.nc = nc; q.dtype = dtype;
    return q;
}
template <typename real>
static StepParams<real> sizes_only(const StepParams<real> &sp)
{
    const mpc_lqr_problem q = sizes_only(sp.B, sp.T, sp.ns, sp.nc, sizeof(real) == 4 ? MPC_F32 : MPC_F64);
    StepParams<real> s = make_params<real>(&q, nullptr, nullptr);
    s.env.kind = sp.env.kind;
    return s;
}
// ... and the caller's blocks where the problem names them: pointers and strides of C, c, F, f, x_init and the nominal (a problem of
// sizes alone has none, and so sits on every grid).  Default options still.
template <typename real>
static StepParams<real> sizes_and_blocks(const StepParams<real> &sp)
{
    StepParams<real> s = sizes_only(sp);
    s.x_init = sp.x_init; s.cur_x = sp.cur_x; s.cur_u = sp.cur_u;
    s.C = sp.C; s.C_st = sp.C_st; s.C_sb = sp.C_sb; s.c = sp.c; s.c_st = sp.c_st; s.c_sb = sp.c_sb;
    s.F = sp.F; s.F_st = sp.F_st; s.F_sb = sp.F_sb; s.f = sp.f; s.f_st = sp.f_st; s.f_sb = sp.f_sb;
    return s;
}

// What a kernel keeps in the workspace, in bytes from its start (-1: not there): the gains K | k where the caller passes none, its own
// record Kk, all it asks for (`bytes`), and the k_t of its box QPs a later step may start from (qp: byte offset, element strides).
// One function per layout; e = sizeof(real), TB = T B.
struct WsLayout { int64_t K, k, Kk, bytes, qp, qp_st, qp_sb; };
// the generic kernels: K [T,B,nc,ns] | k [T,B,nc]
static WsLayout layout_generic(int64_t TB, int B, int ns, int nc, int64_t e) { return {0, TB * nc * ns * e, -1, TB * nc * (ns + 1) * e, -1, 0, 0}; }
// one lane per problem; gains parked as [T][ns+1][B], behind them one trajectory column [T][ns+1] per line-search trial lane (<= 8 per
// problem): 9 (ns + 1) reals per problem-step <= 504 bytes
static WsLayout layout_row(int64_t TB, int B, int ns, int nc, int64_t e) { return {0, TB * nc * ns * e, 0, TB * nc * (ns + 1) * e * 9, -1, 0, 0}; }
// the fused kernels park their gains [T,B,64] in the workspace; float32: gain record + (m, M) record + the second line-search trial's
// trajectory (box-constrained 12/4 kernel); the 12/4 kernel's gain record Kk[t][b][lane 0..15][4]: lane 12 holds k
static WsLayout layout_fused12(int64_t TB, int B, int ns, int nc, int64_t e) { return {0, TB * nc * ns * e, 0, e == 4 ? TB * (128 + 16) * 4 : TB * 64 * 8, -1, 0, 0}; }
static WsLayout layout_dpp16(int64_t TB, int B, int ns, int nc, int64_t e) { return {0, TB * nc * ns * e, 0, layout_fused12(TB, B, ns, nc, e).bytes, 48 * 4, (int64_t)B * 64, 64}; }
// the constrained modes park (M, Quu, m) [T,B,328] + the second trial's trajectory [T,B,40] behind the gains, for the rollout that
// prices without C
static WsLayout layout_mfma40(int64_t TB, int B, int ns, int nc, int64_t e)
{
    const WsLayout w = layout_generic(TB, B, ns, nc, e);
    return {w.K, w.k, w.bytes, w.bytes + TB * (328 + 40) * 4, w.k, (int64_t)B * nc, nc};
}
// the kernel's own padded gains K [T,B,8,32] | k [T,B,8] (entries >= n_ctrl zero) | (M, Quu, m) [T,B,328] | second trial [T,B,40]
// (the narrow instantiation lives inside this layout: its gains K [T,B,8,16] in the front half of the K region, k where the padded kernel
// keeps it -- the record a later step starts from is the same --, (M, Quu, m) [T,B,200] | [T,B,24] in Kk)
static WsLayout layout_pad40(int64_t TB, int B, int ns, int nc, int64_t e)
{
    const int64_t k = TB * 256 * 4, Kk = k + TB * 8 * 4;
    return {0, k, Kk, Kk + TB * (328 + 40) * 4, k, (int64_t)B * 8, 8};
}

// A lane per problem leaves the chip empty at the batch sizes iLQR is run at (B = 1024: 16 .. 128 wavefronts
// on 1024 SIMDs) and its time is one lane's instruction count times the horizon; a 16-lane row per problem
// does everything that is independent over t for 16 timesteps at once and every line-search trial at once.
// Worth its sixteen lanes while all its wavefronts are resident together, at most two to a SIMD (measured,
// profiles/r03_experiments.md section 6: pendulum up to B = 8192, cart-pole -- 39.6 KB of LDS per wavefront --
// up to 4096; twice that and the lane-per-problem kernel is level or ahead).
static bool row_kernel_pays(long lds_bytes, int B)          // lds_bytes: of one wavefront (four problems)
{
    const long per_cu = (160L * 1024) / lds_bytes;
    return (B + 3) / 4 <= (device_facts().simds / 4) * (per_cu < 8 ? per_cu : 8);
}
static bool wave1_pays(const StepParams<float> &sp) { return wave1_supported(sp) && row_kernel_pays(wave1_lds_bytes(sp), sp.B); }
static bool wave1_pays(const StepParams<double> &) { return false; }
// ... the same rule for the carry instantiation (impl 10, forced only: mpc_lqr_row_carry_pays tells a caller where to force it)
static bool wave1_carry_pays(const StepParams<float> &sp) { return wave1_carry_supported(sp) && row_kernel_pays(wave1_carry_lds_bytes(sp), sp.B); }

// ring depth of the 12/4 kernel (lqr_dpp16.hip): the unconstrained step always on the short ring; the constrained one there
// only when the batch has more waves (4 problems each) than the chip has SIMDs (256 CUs x 4)
static int dpp16_ring(const StepParams<float> &sp)
{
    const bool constrained = sp.bound_mode != MPC_BOUND_NONE || sp.zero_mask != nullptr;
    const int force = env_switch(SW_DPP16_RING, device_facts().ring_force);
    return (force ? force == 2 : (!constrained || (sp.B + 3) / 4 > device_facts().simds)) ? 2 : 4;
}
static int launch_dpp16(const StepRoute &r, const StepParams<float> &q, hipStream_t st)
{
    // (the route's answer stays "impl 3, ring 2": the resident-F build is the same kernel with the same results, bit for bit)
    if (r.ring == 2 && dpp16_resident(q)) {
        g_resident_launches.fetch_add(1, std::memory_order_relaxed);
        return launch_step_dpp16_res(q, st);
    }
    return r.ring == 2 ? launch_step_dpp16_ring2(q, st) : launch_step_dpp16(q, st);
}

// One row per kernel, step_kernels[MPC_IMPL_*]: all the router knows about it.  The families are the placement blocks of step_route.
enum StepFamily { FAM_NONE, FAM_GENERIC, FAM_ROW /* a lane or a row per problem */, FAM_FUSED12 /* 12/4-class fused, gains optional */,
                  FAM_MFMA40 /* 32/8 exact */, FAM_PAD40 /* 32/8 padded, narrow */ };
enum {
    K_SIMULATOR = 1,        // takes a simulator as true_dynamics
    K_CARRIES = 2,          // ... and one behind MPC_ENV_CTRL_CARRY
    K_CARRY_ONLY = 4,       // ... and nothing else (so: a whole step only)
    K_SWEEP_STOP = 8,       // can stop after its sweep (MPC_OPT_SWEEP_ONLY); a call heading for any other kernel takes the generic sweep
    K_PARKS_STATUS = 16,    // its layout counts where a caller's missing status words are parked (status_scratch_offset)
    K_SIZES_QUERY = 32,     // its rule looks at the tensors and the options: a query (mpc_lqr_impl_supported) is answered from the sizes
                            // and from the blocks the problem names (alignment of pointers and strides), the options left out as ever
    K_SIZES_RECORD = 64,    // ... and so is mpc_lqr_qp_record for a call that forces it
};
struct StepRefusal { int code; const char *text; };
template <typename real>
struct StepKernelIn {                                                 // a kernel in one dtype
    bool (*rule)(const StepParams<real> &);                           // its own rule (lqr_*.hip); NULL: it does not exist in this dtype
    int (*launch)(const StepRoute &, const StepParams<real> &, hipStream_t);      // picks the build variant from (route, params)
    bool needs_workspace;                                             // takes the call only with room in an aligned workspace
    int (*ring)(const StepParams<real> &);                            // its sweep ring, where it has more than one
    StepRefusal refused;                                              // what a forced call it does not take is told (NULL: the call goes on)
};
struct StepKernel {
    int code; const char *name; StepFamily family;
    int auto_rank;                               // its place in the order impl 0 proposes kernels in; 0: never proposed by that order
    unsigned flags;                              // K_*
    WsLayout (*layout)(int64_t TB, int B, int ns, int nc, int64_t e);
    StepKernelIn<float> f32;
    StepKernelIn<double> f64;
    // what a forced call is told at once: in a dtype the kernel does not exist in (NULL: see `refused`), off its shapes, and with (or,
    // K_CARRY_ONLY, without) a simulator
    const char *no_dtype, *no_shape, *no_simulator;
};
typedef StepParams<float> P32;
// launchers and rules that need a word more than the kernel's own: a kernel with one build, the generic kernels, the one-control shapes
template <typename real, int (*launch)(const StepParams<real> &, hipStream_t)>
static int one_build(const StepRoute &, const StepParams<real> &q, hipStream_t st) { return launch(q, st); }
template <typename real>
static int launch_generic(const StepRoute &r, const StepParams<real> &q, hipStream_t st) { return launch_step_generic<real>(q, r.phase, st); }
template <typename real>
static bool generic_fits(const StepParams<real> &s) { return generic_lds_bytes(s.ns, s.nc, sizeof(real)) <= 160 * 1024; }
template <typename real>
static bool is_tiny(const StepParams<real> &s) { return tiny_supported(s.ns, s.nc); }
static const char ws_small[] = "workspace too small (see mpc_lqr_workspace_bytes)";
static const char ws_small_or_off[] = "workspace too small or not 16-byte aligned (see mpc_lqr_workspace_bytes)";
static const char both_gains[] = "pass both K and k, or neither";
static const char generic_only[] = "a simulator as true_dynamics runs on the generic kernels only";
static const char lane_shapes[] = "lane-per-problem / wavefront-per-problem kernel needs n_ctrl = 1, n_state <= 6";
static const char wave4_fp32[] = "the 4-problems-per-wave kernel is fp32 only";
static const char row_rule[] = "the row-per-problem kernel is float32, max_linesearch_iter <= 16, four problems in 150 KiB of LDS";
static constexpr StepKernel step_kernels[] = {
    {MPC_IMPL_AUTO, "auto", FAM_NONE, 0, 0, layout_generic},         // (nobody: also an unknown code)
    {MPC_IMPL_GENERIC, "generic", FAM_GENERIC, 0, K_SIMULATOR | K_PARKS_STATUS, layout_generic,
     {generic_fits<float>, launch_generic<float>}, {generic_fits<double>, launch_generic<double>}},
    // float64 (round 5, v_mfma_f64_16x16x4_f64) only with its workspace: a caller written against ABI 7 -- out->K / out->k given, no or
    // a small workspace -- keeps the generic kernel under impl 0
    {MPC_IMPL_MFMA16, "mfma16", FAM_FUSED12, 3, K_PARKS_STATUS, layout_fused12,
     {mfma16_supported, one_build<float, launch_step_mfma16>, false, nullptr,
      {MPC_E_DIMS, "fused MFMA kernel needs fp32, n_state <= 12, n_ctrl <= 4, max_linesearch_iter <= 16"}},
     {mfma16_supported, one_build<double, launch_step_mfma16>, true, nullptr,
      {MPC_E_DIMS, "fused MFMA kernel needs n_state <= 12, n_ctrl <= 4, max_linesearch_iter <= 16"}},
     nullptr, nullptr, generic_only},
    {MPC_IMPL_DPP16, "dpp16", FAM_FUSED12, 1, K_SWEEP_STOP | K_PARKS_STATUS | K_SIZES_QUERY, layout_dpp16,
     {dpp16_supported, launch_dpp16, false, dpp16_ring, {MPC_E_DIMS, "DPP kernel needs fp32, n_state = 12, n_ctrl = 4 and 16-byte aligned blocks"}},
     {nullptr, nullptr, false, nullptr, {MPC_E_DTYPE, wave4_fp32}}, nullptr, nullptr, generic_only},
    {MPC_IMPL_TINY, "tiny", FAM_ROW, 0, K_SIMULATOR | K_CARRIES | K_PARKS_STATUS, layout_row,
     {is_tiny<float>, one_build<float, launch_step_tiny<float>>}, {is_tiny<double>, one_build<double, launch_step_tiny<double>>},
     nullptr, lane_shapes},
    // n_state = 32, n_ctrl = 8: register-resident MFMA sweep and rollout (lqr_mfma40_body.h)
    {MPC_IMPL_MFMA40, "mfma40", FAM_MFMA40, 4, K_SWEEP_STOP | K_PARKS_STATUS | K_SIZES_QUERY | K_SIZES_RECORD, layout_mfma40,
     {mfma40_supported, [](const StepRoute &r, const P32 &q, hipStream_t st) { return r.ring == 2 ? launch_step_mfma40_ring2(q, st) : launch_step_mfma40(q, st); },
      false, mfma40_ring, {MPC_E_DIMS, "MFMA kernel needs fp32, n_state = 32, n_ctrl = 8, 16-byte aligned blocks, no simulator"}},
     {nullptr, nullptr, false, nullptr, {MPC_E_DTYPE, "the MFMA sweep is fp32 only"}}},
    {MPC_IMPL_WAVE1, "wave1", FAM_ROW, 0, K_SIMULATOR | K_PARKS_STATUS, layout_row,
     {[](const P32 &s) { return is_tiny(s) && wave1_supported(s); }, one_build<float, launch_step_wave1>, false, nullptr, {MPC_E_DIMS, row_rule}},
     {nullptr, nullptr, false, nullptr, {MPC_E_DIMS, row_rule}}, nullptr, lane_shapes},
    // with the workspace only: its padded gains and the constrained modes' records, 16-byte aligned
    {MPC_IMPL_MFMA40_PAD, "mfma40_pad", FAM_PAD40, 5, K_SWEEP_STOP | K_PARKS_STATUS, layout_pad40,
     {mfma40_pad_supported, [](const StepRoute &r, const P32 &q, hipStream_t st) { return r.pad16 ? launch_step_mfma40_pad16(q, st) : launch_step_mfma40_pad4(q, st); },
      true, nullptr, {MPC_E_DIMS, "padded MFMA kernel needs fp32, n_state <= 32, n_ctrl <= 8, max_linesearch_iter <= 16, no simulator, and the "
                                  "workspace of mpc_lqr_workspace_bytes (16-byte aligned)"}}},
    {MPC_IMPL_DPP16_PAD, "dpp16_pad", FAM_FUSED12, 2, K_SWEEP_STOP | K_PARKS_STATUS, layout_fused12,
     {dpp16_pad_supported, one_build<float, launch_step_dpp16_pad>, false, nullptr,
      {MPC_E_DIMS, "padded DPP kernel needs fp32, n_state <= 12, n_ctrl <= 4, max_linesearch_iter <= 16"}},
     {nullptr, nullptr, false, nullptr, {MPC_E_DTYPE, wave4_fp32}}, nullptr, nullptr, generic_only},
    // (impl 9, the padded kernel's narrow instantiation, and impl 10, the row kernel's for a simulator behind the flag -- a plain
    // simulator or a linear model has impl 6: forced only, and outside the parked-status offset callers have always been handed)
    {MPC_IMPL_MFMA40_NARROW, "mfma40_narrow", FAM_PAD40, 0, K_SWEEP_STOP, layout_pad40,
     {mfma40_narrow_supported, [](const StepRoute &r, const P32 &q, hipStream_t st) { return r.pad16 ? launch_step_mfma40_narrow16(q, st) : launch_step_mfma40_narrow4(q, st); },
      true, nullptr, {MPC_E_DIMS, "narrow MFMA kernel needs fp32, n_state <= 16, n_ctrl <= 8, max_linesearch_iter <= 16, no simulator, and the "
                                  "workspace of mpc_lqr_workspace_bytes (16-byte aligned)"}},
     {}, "the narrow MFMA kernel is fp32 only"},
    {MPC_IMPL_WAVE1_CARRY, "wave1_carry", FAM_ROW, 0, K_SIMULATOR | K_CARRIES | K_CARRY_ONLY, layout_row,
     {[](const P32 &s) { return is_tiny(s) && wave1_carry_supported(s); }, one_build<float, launch_step_wave1_carry>, false, nullptr,
      {MPC_E_DIMS, "the row-per-problem carry kernel is float32, max_linesearch_iter <= 16, four problems in 150 KiB of LDS"}},
     {}, "the row-per-problem carry kernel is fp32 only", "the row-per-problem carry kernel needs a whole step with n_ctrl = 1, n_state = 4 or 6",
     "the row-per-problem carry kernel needs a simulator behind MPC_ENV_CTRL_CARRY as true_dynamics"},
};
constexpr int N_STEP_KERNELS = sizeof(step_kernels) / sizeof(step_kernels[0]);
constexpr bool step_kernels_in_place(int i = 0) { return i == N_STEP_KERNELS || (step_kernels[i].code == i && step_kernels_in_place(i + 1)); }
static_assert(N_STEP_KERNELS == MPC_IMPL_WAVE1_CARRY + 1 && step_kernels_in_place(), "step_kernels[code] is the row of `code`");

// The order impl 0 proposes kernels in, off the ranks: 12/4 on its own kernel; every other float32 shape up to 12/4, and 12/4 itself where
// a block is not 16-byte aligned, on that kernel's PADDED instantiation (round 6; ahead of the one-problem-per-wavefront kernel that
// served them in rounds 1-5 and still serves float64: what every test and gradient check of the reference runs in, tests/test_mpc.py
// .double()); 32/8 on its own kernel; every float32 shape up to 32/8 that has no kernel of its own (13/4, 20/5, 24/8, 32/4, 8/6 ...) on
// the 32/8 kernel's PADDED instantiation (lqr_mfma40_body.h, PADK) -- the reference's sweep is shape-agnostic (mpc/lqr_step.py:61-158),
// and between the hand-tuned shapes the generic kernel ran at 4 % of the roofline (missing 1).
struct StepOrder { int n, code[N_STEP_KERNELS]; };
constexpr StepOrder step_order_of_ranks()
{
    StepOrder o = {};
    for (int rank = 1; rank < N_STEP_KERNELS; ++rank)
        for (const StepKernel &k : step_kernels)
            if (k.auto_rank == rank) o.code[o.n++] = k.code;
    return o;
}
static constexpr StepOrder step_auto_order = step_order_of_ranks();

static bool known_kernel(int kernel) { return kernel > MPC_IMPL_AUTO && kernel < N_STEP_KERNELS; }
template <typename real>
static const StepKernelIn<real> &in_dtype(const StepKernel &k) { if constexpr (sizeof(real) == 4) return k.f32; else return k.f64; }
// Does the kernel take this call, by its own rule?  query: sizes, dtype and options -- the alignment of the tensors is checked at launch.
template <typename real>
static bool kernel_takes(const StepKernel &k, const StepParams<real> &sp, bool query = false)
{
    const StepKernelIn<real> &d = in_dtype<real>(k);
    return d.rule && d.rule(query && (k.flags & K_SIZES_QUERY) ? sizes_and_blocks(sp) : sp);
}
template <typename real>
static WsLayout ws_layout(int kernel, int T, int B, int ns, int nc) { return step_kernels[kernel].layout((int64_t)T * B, B, ns, nc, sizeof(real)); }

// where a caller's missing status array lives inside the workspace: behind the largest layout among the kernels the shape can reach
// -- and never in front of the float32 12/4-class record, whatever the shape and dtype (the size callers have always been handed)
template <typename real>
static int64_t largest_layout(const mpc_lqr_problem *p)
{
    const mpc_lqr_problem q = sizes_only(p->B, p->T, p->ns, p->nc, p->dtype);
    const StepParams<real> s = make_params<real>(&q, nullptr, nullptr);
    int64_t m = ws_layout<float>(MPC_IMPL_DPP16, p->T, p->B, p->ns, p->nc).bytes;
    for (const StepKernel &k : step_kernels) {
        if (!(k.flags & K_PARKS_STATUS)) continue;
        const int64_t b = ws_layout<real>(k.code, p->T, p->B, p->ns, p->nc).bytes;
        if ((k.family == FAM_GENERIC || kernel_takes<real>(k, s, true)) && b > m) m = b;
    }
    return m;
}
static int64_t status_scratch_offset(const mpc_lqr_problem *p)
{
    return ((p->dtype == MPC_F64 ? largest_layout<double>(p) : largest_layout<float>(p)) + 15) & ~(int64_t)15;
}

// Which kernel takes this call, and where its pieces live in the workspace.  Launches nothing, sets no error state, allocates
// nothing; never cached (the answer depends on the pointers and, with MPC_DPP16_RING_DYNAMIC, on the environment).  The checks of the
// call, then one block per family: what a call that forces a kernel of the family is refused with, and where a call heading for one
// (forced or under impl 0) finds its pieces.  The order in which refusals fire is part of the interface.
template <typename real>
StepRoute step_route(const StepParams<real> &sp, const mpc_lqr_problem *p, int impl, int phase_mask, const void *workspace,
                     int64_t workspace_bytes)
{
    constexpr bool f32 = sizeof(real) == 4;
    StepRoute r = {0, nullptr, 0, phase_mask, 0, false, false, -1, -1, -1, -1, -1, 0, 0};
    const auto refuse = [&r](int code, const char *msg) { r.code = code; r.msg = msg; return r; };
    const bool step = phase_mask == 3, aligned = (uintptr_t)workspace % 16 == 0, tiny = tiny_supported(sp.ns, sp.nc), forcing = impl != MPC_IMPL_AUTO;
    const auto room = [&](int64_t bytes) { return workspace && workspace_bytes >= bytes; };
    const auto layout = [&](int kernel) { return ws_layout<real>(kernel, sp.T, sp.B, sp.ns, sp.nc); };
    // a kernel takes the call: by its own rule; with a simulator only where it runs one; and with the workspace where the call falls
    // through to the next kernel without it
    const auto takes_now = [&](const StepKernel &k) {
        if (!kernel_takes<real>(k, sp)) return false;
        if (sp.env.kind && !(k.flags & K_SIMULATOR)) return false;
        return !in_dtype<real>(k).needs_workspace || (room(layout(k.code).bytes) && aligned);
    };
    signed char asked[N_STEP_KERNELS];           // each kernel is asked once per call
    memset(asked, -1, sizeof(asked));
    const auto takes = [&](int kernel) {
        if (!known_kernel(kernel)) return false;
        if (asked[kernel] < 0) asked[kernel] = takes_now(step_kernels[kernel]);
        return asked[kernel] != 0;
    };
    const auto family_takes = [&](StepFamily family) {
        for (const StepKernel &k : step_kernels)
            if (k.family == family && takes(k.code)) return true;
        return false;
    };
    // a fused kernel took the call: under impl 0 the problems it flags MPC_ST_C_ASYMMETRIC are solved again (resolve_asymmetric)
    const auto fused = [&](int kernel, const WsLayout &w) { r.kernel = kernel; r.Kk_off = w.Kk; r.needs_resolve = !forcing && !sp.c_symmetric; return r; };
    const auto record = [&r](const WsLayout &w) { r.qp_off = w.qp; r.qp_st = w.qp_st; r.qp_sb = w.qp_sb; };

    // The kernel the call is heading for: the forced one, or under impl 0 the one-control shapes up to six states on the lane- /
    // row-per-problem kernels, whichever pays; the first of step_auto_order that takes any other; everything else on the generic kernels.
    int kernel = impl;
    if (!forcing) {
        kernel = MPC_IMPL_GENERIC;
        if (step && tiny) kernel = wave1_pays(sp) ? MPC_IMPL_WAVE1 : MPC_IMPL_TINY;
        else if (step)
            for (int i = 0; i < step_auto_order.n; ++i)
                if (takes(step_auto_order.code[i])) { kernel = step_auto_order.code[i]; break; }
    }
    const StepKernel &heading = step_kernels[known_kernel(kernel) ? kernel : MPC_IMPL_AUTO];
    const StepKernelIn<real> &mine = in_dtype<real>(heading);

    // the symmetry verdict travels in the status words: a caller that passes none gets them parked behind the workspace
    if (!sp.status && step && workspace) {
        const int64_t off = status_scratch_offset(p);
        if (workspace_bytes >= off + (int64_t)sp.B * 4) r.status_off = off;
    }
    if ((phase_mask & 2) && !sp.sweep_only && (!sp.new_x || !sp.new_u)) return refuse(MPC_E_NULL, "new_x / new_u is NULL");
    if (sp.sweep_only) {
        if (!step) return refuse(MPC_E_ARG, "MPC_OPT_SWEEP_ONLY is an option of mpc_lqr_step");
        if (!sp.K || !sp.k) return refuse(MPC_E_NULL, "MPC_OPT_SWEEP_ONLY needs out->K and out->k");
        if (sp.env.kind) return refuse(MPC_E_ARG, "MPC_OPT_SWEEP_ONLY with a simulator as true_dynamics");
        if (!((heading.flags & K_SWEEP_STOP) && takes(kernel))) {
            if (forcing && heading.family != FAM_GENERIC) return refuse(MPC_E_ARG, "MPC_OPT_SWEEP_ONLY: this kernel cannot stop after its sweep");
            r.kernel = MPC_IMPL_GENERIC; r.phase = 1;
            return r;
        }
    }
    // MPC_ENV_CTRL_CARRY: the lane-per-problem kernel carries the control (lqr_tiny_body.h), and so does the row-per-problem kernel's
    // carry instantiation (forced only); the row-per-problem and the generic kernels call the simulator as it is and REFUSE the
    // flag -- never a silent un-augmented answer
    if (sp.env.carry && (!step || (forcing && !(heading.flags & K_CARRIES))))
        return refuse(MPC_E_UNSUPPORTED, "MPC_ENV_CTRL_CARRY: only mpc_lqr_step on the lane-per-problem kernel (impl 0 or 4) carries the control");
    if (sp.env.kind && sp.env.linearize && !(step && tiny && (!forcing || heading.family == FAM_ROW)))
        return refuse(MPC_E_ARG, "in-kernel linearisation needs the lane-per-problem kernel (n_ctrl = 1, n_state <= 6)");
    if (forcing && !mine.rule && heading.no_dtype) return refuse(MPC_E_DTYPE, heading.no_dtype);

    // A lane or a row per problem.  (These kernels keep Q and V as general matrices, like the reference: nothing to test or re-solve.)
    if (heading.family == FAM_ROW) {
        if (forcing) {
            if (!step || !tiny) return refuse(MPC_E_DIMS, heading.no_shape);
            if ((heading.flags & K_CARRY_ONLY) && !(sp.env.kind && sp.env.carry)) return refuse(MPC_E_ARG, heading.no_simulator);
            if (mine.refused.text && !takes(kernel)) return refuse(mine.refused.code, mine.refused.text);
        }
        const WsLayout w = layout(kernel);
        if (!room(w.bytes)) return refuse(MPC_E_ARG, ws_small);
        r.kernel = kernel; r.Kk_off = w.Kk;
        return r;
    }

    // The 12/4 class: out->K / out->k are optional on its three kernels, which share the size of their workspace.  Whoever the call is
    // heading for -- the forced generic kernel and a simulator apart --, float32 insists on the pair of gains and, where one of the three
    // takes the call, on their workspace; float64 hands the call to the fused kernel wherever that takes it (a forced 5 or 7 as well).
    if (heading.family == FAM_FUSED12 && sp.env.kind) return refuse(MPC_E_ARG, heading.no_simulator);
    if (step && !(forcing && heading.family == FAM_GENERIC) && !sp.env.kind) {
        const bool half_gains = (sp.K == nullptr) != (sp.k == nullptr), heading12 = heading.family == FAM_FUSED12, forced12 = forcing && heading12;
        if constexpr (f32) {
            if (half_gains) return refuse(MPC_E_NULL, both_gains);
            if (forced12 && !takes(kernel)) return refuse(mine.refused.code, mine.refused.text);
            if (heading12 || family_takes(FAM_FUSED12)) {
                const WsLayout w = layout(heading12 ? kernel : MPC_IMPL_MFMA16);      // (`bytes` is the same for the three)
                if (!(room(w.bytes) && aligned)) return refuse(MPC_E_ARG, ws_small_or_off);
                if (heading12) {
                    if (mine.ring) r.ring = mine.ring(sp);
                    record(w);
                    return fused(kernel, w);
                }
            }
        } else {
            if (forced12 && !kernel_takes<real>(heading, sp)) return refuse(mine.refused.code, mine.refused.text);
            if (forced12 && !takes(kernel)) return refuse(MPC_E_ARG, ws_small_or_off);     // (only a FORCED fused kernel insists on its workspace)
            if (takes(MPC_IMPL_MFMA16)) {
                if (half_gains) return refuse(MPC_E_NULL, both_gains);
                return fused(MPC_IMPL_MFMA16, layout(MPC_IMPL_MFMA16));
            }
        }
    }

    // The 32/8 kernel's padded and narrow instantiations, on their own padded gains (float64 has neither: a forced 7 goes on).
    if constexpr (f32) {
        if (heading.family == FAM_PAD40) {
            if (forcing && !(step && takes(kernel))) return refuse(mine.refused.code, mine.refused.text);
            const WsLayout w = layout(kernel);
            r.K_off = w.K; r.k_off = w.k; r.pad16 = mfma40_pad16_supported(sp);
            record(w);
            return fused(kernel, w);
        }
    }

    // Everybody else works on the gains K | k of the generic layout: the caller's, or parked in the workspace.
    if (!sp.K || !sp.k) {
        const WsLayout w = layout(MPC_IMPL_GENERIC);
        if (!step) return refuse(MPC_E_NULL, "K / k is NULL");
        if (!room(w.bytes)) return refuse(MPC_E_ARG, ws_small);
        r.K_off = w.K; r.k_off = w.k;
    }
    if (heading.family == FAM_MFMA40) {
        if (forcing && !(step && takes(kernel))) return refuse(mine.refused.code, mine.refused.text);
        WsLayout w = layout(kernel);
        // (M, Quu, m) record of the constrained modes: behind K | k where the workspace has the room (rollout_priced)
        if (!((sp.bound_mode != MPC_BOUND_NONE || sp.zero_mask) && room(w.bytes) && aligned)) w.Kk = -1;
        r.ring = mine.ring(sp);
        if (r.K_off >= 0) record(w);
        return fused(kernel, w);
    }
    r.kernel = MPC_IMPL_GENERIC;
    return r;
}

// (instantiated here, and so visible in the library, for tests/step_route_probe.cpp alone, which prints the whole route on the host:
// an internal C++ template over StepParams, NOT part of the API -- that is include/mpc_lqr.h, and mpc_lqr_step_route is its query)
template StepRoute step_route<float>(const StepParams<float> &, const mpc_lqr_problem *, int, int, const void *, int64_t);
template StepRoute step_route<double>(const StepParams<double> &, const mpc_lqr_problem *, int, int, const void *, int64_t);

// After a fused kernel under impl = 0 (auto): the problems it flagged MPC_ST_C_ASYMMETRIC are solved again by the generic
// kernels, which use C exactly as the reference does (mpc/lqr_step.py:68, 294); everything else is left as it is.  A
// compact grid reads the flags -- no host round trip, nothing to synchronise on.
template <typename real>
static int resolve_asymmetric(StepParams<real> sp, void *workspace, hipStream_t st)
{
    if (!sp.status) return MPC_OK;
    if (sp.env.kind && sp.env.linearize) return MPC_OK;      // no F, f arrays to fall back on: the bit is the answer
    sp.gate = sp.status;
    sp.Kk = nullptr;
    if (!sp.K || !sp.k) {
        const WsLayout w = ws_layout<real>(MPC_IMPL_GENERIC, sp.T, sp.B, sp.ns, sp.nc);
        sp.K = (real *)((char *)workspace + w.K);
        sp.k = (real *)((char *)workspace + w.k);
    }
    return launch_step_generic<real>(sp, sp.sweep_only ? 1 : 3, st);
}

// one launch per kernel
template <typename real>
static int launch_routed(const StepRoute &r, const StepParams<real> &q, hipStream_t st)
{
    const auto launch = known_kernel(r.kernel) ? in_dtype<real>(step_kernels[r.kernel]).launch : nullptr;
    return launch ? launch(r, q, st) : MPC_E_ARG;
}

// mpc_lqr_options.qp_start is a hint: an array the staging DMAs cannot fetch (16-byte granules) is ignored, not an error
template <typename real>
static void filter_qp_start(StepParams<real> &sp)
{
    if (sp.qp_start && (sp.bound_mode == MPC_BOUND_NONE || (uintptr_t)sp.qp_start % 16 || sp.qp_start_st % 4 || sp.qp_start_sb % 4 ||
                        sp.qp_start_st < 0 || sp.qp_start_sb < 0 || sp.qp_start_st * 4 >= (1ll << 32) || sizeof(real) != 4))
        sp.qp_start = nullptr;
}

template <typename real>
static int step_impl(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_lqr_outputs *out,
                     void *workspace, int64_t workspace_bytes, int impl, int phase_mask,
                     const void *old_costs_in, hipStream_t st)
{
    StepParams<real> sp = make_params<real>(p, o, out);
    sp.old_costs_in = (const real *)old_costs_in;
    filter_qp_start(sp);
    const StepRoute r = step_route(sp, p, impl, phase_mask, workspace, workspace_bytes);
    if (r.code) return fail(r.code, r.msg);
    const auto at = [workspace](int64_t off) { return off < 0 ? nullptr : (char *)workspace + off; };
    if (r.status_off >= 0) sp.status = (int *)at(r.status_off);
    real *const K_caller = sp.K, *const k_caller = sp.k;
    sp.Kk = (real *)at(r.Kk_off);
    if (r.K_off >= 0) {                          // gains where the route put them
        if (step_kernels[r.kernel].family == FAM_PAD40) { sp.K_user = sp.K; sp.k_user = sp.k; }
        sp.K = (real *)at(r.K_off);
        sp.k = (real *)at(r.k_off);
    }
    const int rc = launch_routed(r, sp, st);
    if (rc || !r.needs_resolve) return rc;
    sp.K = K_caller; sp.k = k_caller; sp.K_user = sp.k_user = nullptr;      // the re-solve writes the caller's gains, or parks its own
    return resolve_asymmetric(sp, workspace, st);
}

// the argument checks of mpc_lqr_step, and of mpc_lqr_step_route, which answers for the same arguments
// (whole_step false: of mpc_lqr_sweep and mpc_lqr_rollout, which have no in-kernel linearisation and so always need F)
static int check_step(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_lqr_outputs *out, bool whole_step = true)
{
    const bool inline_lin = whole_step && o && o->true_dynamics && o->true_dynamics->linearize;
    int rc = check_problem(p, true, true, !inline_lin);
    if (rc) return rc;
    if ((rc = check_options(p, o))) return rc;
    if (!out) return fail(MPC_E_NULL, "outputs is NULL");
    return MPC_OK;
}

// mpc_lqr_sweep (phase 1) and mpc_lqr_rollout (phase 2): the generic kernels, the gains the caller's
static int sweep_or_rollout(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_lqr_outputs *out, int phase, const void *old_costs_in,
                            void *stream)
{
    const int rc = check_step(p, o, out, false);
    if (rc) return rc;
    if (p->B == 0) return MPC_OK;
    hipStream_t st = (hipStream_t)stream;
    return p->dtype == MPC_F32 ? step_impl<float>(p, o, out, nullptr, 0, MPC_IMPL_GENERIC, phase, old_costs_in, st)
                               : step_impl<double>(p, o, out, nullptr, 0, MPC_IMPL_GENERIC, phase, old_costs_in, st);
}

template <typename real>
static int route_query(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_lqr_outputs *out, const void *workspace,
                       int64_t workspace_bytes, int impl, int *ring)
{
    StepParams<real> sp = make_params<real>(p, o, out);
    filter_qp_start(sp);
    const StepRoute r = step_route(sp, p, impl, 3, workspace, workspace_bytes);
    if (r.code) return fail(r.code, r.msg);
    if (ring) *ring = r.ring;
    return r.kernel;
}

// ---------------------------------------------------------------------------------------------------------------------
// The kernels behind the KKT backward (MPC_KKT_*, MPC_KKT_GRADS_*, include/mpc_lqr.h): what each one takes, the workspace it lives
// in, and -- kkt_fused_route, kkt_grads_route -- which of them takes a call.  mpc_lqr_kkt_fused, its two queries and
// mpc_lqr_kkt_fused_route, mpc_lqr_kkt_grads and mpc_lqr_kkt_grads_route all ask here.
// ---------------------------------------------------------------------------------------------------------------------

// Does fused kernel `kernel` take this call, by its own rule (lqr_dpp16.hip, lqr_mfma40.hip)?  query: the form
// mpc_lqr_kkt_fused_supported asks -- sizes, dtype (the caller's: these kernels are float32) and flags; the rules are then asked
// with no tensors, so every block counts as aligned.
static bool kkt_kernel_takes(int kernel, const StepParams<float> &sp, const KktPointers &a, bool query = false)
{
    // (u_zero_I and delta_u of the FORWARD are not inputs of the backward: the reference's nested solve is built from the bounds
    // alone, `u_zero_I = I` from u* and the bounds, `delta_u = None`, mpc/lqr_step.py:322-340 -- the launchers drop them; rounds
    // 1-3 refused such options here and the caller fell to three launches for nothing)
    if (!sp.c_symmetric || sp.env.kind) return false;
    if (query) {
        StepParams<float> s = sizes_only(sp);
        s.c_symmetric = 1;
        return kkt_kernel_takes(kernel, s, KktPointers());
    }
    const float *gx = (const float *)a.dl_dx, *gu = (const float *)a.dl_du, *dC = (const float *)a.dC, *dF = (const float *)a.dF,
                *ws = (const float *)a.workspace;
    switch (kernel) {
    case MPC_KKT_DPP16: return kkt_fused_dpp16_supported(sp, gx, gu, dC, dF, ws);
    // every other shape up to 12/4, and 12/4 itself where a block is not 16-byte aligned: the padded instantiation (round 6)
    case MPC_KKT_DPP16_PAD: return kkt_fused_dpp16_pad_supported(sp, ws);
    // config 5's shape: the nested step with the costates riding along, then the outer-product kernel (two launches); what the
    // kernel stores through 16-byte rows is the caller's here, not the rule's
    case MPC_KKT_MFMA40:
        return kkt_fused_mfma40_supported(sp, gx, gu, dC, dF, ws) && !(a.dx_out && (((uintptr_t)a.dx_out | (uintptr_t)a.du_out) & 15)) &&
               !((uintptr_t)a.dx_init & 15) && !(a.df && ((uintptr_t)a.df & 15));
    // every other shape up to 32/8, and 32/8 itself off the 16-byte grid: the padded instantiations (round 6)
    case MPC_KKT_MFMA40_PAD16: return kkt_fused_mfma40_pad16_supported(sp, ws);
    case MPC_KKT_MFMA40_PAD4: return kkt_fused_mfma40_pad_supported(sp, ws);
    // the padded instantiations on one state tile (n_state <= 16), in a workspace packed for it: forced only (kkt_fused_route_kernel)
    case MPC_KKT_MFMA40_NARROW16: return kkt_fused_mfma40_narrow16_supported(sp, ws);
    case MPC_KKT_MFMA40_NARROW4: return kkt_fused_mfma40_narrow_supported(sp, ws);
    }
    return false;
}

// The fused kernels in the order they are tried, each with its launcher, the workspace it lives in and what a call that heads for it
// and is taken by nobody is told.  Exact before padded; beyond 12/4 the 16-byte gathers before the dword ones.
typedef int (*KktLaunch)(const StepParams<float> &, const float *, const float *, float *, float *, float *, float *, float *, float *, float *,
                         float *, float, int, hipStream_t);
struct KktKernel {
    int code;
    KktLaunch launch;
    int64_t (*ws_bytes)(int T, int B);       // (a padded instantiation pads to the exact kernel's layout: the same workspace)
    const char *nobody;
    bool forced_only;                        // never proposed by kkt_first: asked for by code or by family (mpc_lqr_kkt_fused_kernel)
    const char *name, *sizes, *views;        // what a call that names this kernel and is refused by it is told
};
static const char kkt_nobody12[] = "mpc_lqr_kkt_fused: the workspace must be 16-byte aligned";
static const char kkt_nobody40[] = "mpc_lqr_kkt_fused: the workspace must be 16-byte aligned (tensor bounds 4-byte aligned)";
static const char kkt_nobody_narrow[] = "mpc_lqr_kkt_fused_kernel: the workspace must be 16-byte aligned (tensor bounds 4-byte aligned)";
static const char kkt_views12[] = "C, c, F, x*, u*, dl_dx, dl_du, dC, dF and the workspace 16-byte aligned, strides multiples of 4";
static const char kkt_views_ws[] = "the workspace 16-byte aligned (tensor bounds 4-byte aligned)";
static const char kkt_views40[] = "every block, output and the workspace 16-byte aligned, strides multiples of 4 (tensor bounds 4-byte aligned)";
static const char kkt_views16[] = "C and F 16-byte aligned with strides multiples of 4, the workspace 16-byte aligned (tensor bounds 4-byte aligned)";
static const KktKernel kkt_order[] = {
    {MPC_KKT_DPP16, launch_kkt_fused_dpp16, kkt_fused_dpp16_workspace_bytes, kkt_nobody12, false,
     "MPC_KKT_DPP16", "n_state = 12, n_ctrl = 4", kkt_views12},
    {MPC_KKT_DPP16_PAD, launch_kkt_fused_dpp16_pad, kkt_fused_dpp16_workspace_bytes, kkt_nobody12, false,
     "MPC_KKT_DPP16_PAD", "n_state <= 12, n_ctrl <= 4", kkt_views_ws},
    {MPC_KKT_MFMA40, launch_kkt_fused_mfma40, kkt_fused_mfma40_workspace_bytes, kkt_nobody40, false,
     "MPC_KKT_MFMA40", "n_state = 32, n_ctrl = 8", kkt_views40},
    {MPC_KKT_MFMA40_PAD16, launch_kkt_fused_mfma40_pad16, kkt_fused_mfma40_workspace_bytes, kkt_nobody40, false,
     "MPC_KKT_MFMA40_PAD16", "n_state <= 32, n_ctrl <= 8, both multiples of 4", kkt_views16},
    {MPC_KKT_MFMA40_PAD4, launch_kkt_fused_mfma40_pad, kkt_fused_mfma40_workspace_bytes, kkt_nobody40, false,
     "MPC_KKT_MFMA40_PAD4", "n_state <= 32, n_ctrl <= 8", kkt_views_ws},
    // one state tile, in their own packed workspace (448 floats a problem-step).  Forced only: the recorded routes of kernel = 0 stay
    {MPC_KKT_MFMA40_NARROW16, launch_kkt_fused_mfma40_narrow16, kkt_fused_mfma40_narrow_workspace_bytes, kkt_nobody_narrow, true,
     "MPC_KKT_MFMA40_NARROW16", "n_state <= 16, n_ctrl <= 8, both multiples of 4", kkt_views16},
    {MPC_KKT_MFMA40_NARROW4, launch_kkt_fused_mfma40_narrow4, kkt_fused_mfma40_narrow_workspace_bytes, kkt_nobody_narrow, true,
     "MPC_KKT_MFMA40_NARROW4", "n_state <= 16, n_ctrl <= 8", kkt_views_ws},
};
static_assert(MPC_KKT_DPP16 == 1 && MPC_KKT_DPP16_PAD == 2 && MPC_KKT_MFMA40 == 3 && MPC_KKT_MFMA40_PAD16 == 4 && MPC_KKT_MFMA40_PAD4 == 5 &&
              MPC_KKT_MFMA40_NARROW16 == 6 && MPC_KKT_MFMA40_NARROW4 == 7 && sizeof(kkt_order) / sizeof(kkt_order[0]) == 7,
              "kkt_order[code - 1] is the row of `code`");

// the first kernel of the order that takes the call (query: its sizes, dtype and flags), or NULL
static const KktKernel *kkt_first(const mpc_lqr_problem *p, const StepParams<float> &sp, const KktPointers &a, bool query = false)
{
    if (p->dtype != MPC_F32) return nullptr;
    for (const KktKernel &k : kkt_order)
        if (!k.forced_only && kkt_kernel_takes(k.code, sp, a, query)) return &k;
    return nullptr;
}

// What every route checks once it knows where the call is heading (the kernel whose workspace it must fit) and who takes its views:
// mpc_lqr_kkt_fused's refusals in its order, then `nobody` where no taker is left (no_kernel: "legal, but no fused kernel").
static KktRoute kkt_route_shared(const mpc_lqr_problem *p, const KktPointers &a, int64_t workspace_bytes, const KktKernel *taker,
                                 const KktKernel *heading, const char *nobody, bool nobody_is_no_kernel)
{
    KktRoute r = {0, nullptr, false, MPC_KKT_NONE, 0};
    const auto refuse = [&r](int code, const char *msg, bool no_kernel = false) { r.code = code; r.msg = msg; r.no_kernel = no_kernel; return r; };
    if (p->B == 0) return r;                     // (the entry succeeds and launches nothing)
    if (!a.dl_dx || !a.dl_du || !a.dC || !a.dc || !a.dx_init) return refuse(MPC_E_NULL, "kkt_fused: NULL argument");
    if (p->T > 1 && !a.dF) return refuse(MPC_E_NULL, "kkt_fused: dF is NULL");
    if ((a.df != nullptr) != (p->f != nullptr && p->T > 1)) return refuse(MPC_E_NULL, "kkt_fused: df goes with f");
    if ((a.dx_out == nullptr) != (a.du_out == nullptr)) return refuse(MPC_E_NULL, "kkt_fused: pass both dx_out and du_out, or neither");
    r.bytes = heading->ws_bytes(p->T, p->B);
    if (!a.workspace || workspace_bytes < r.bytes) return refuse(MPC_E_ARG, "workspace too small (see mpc_lqr_kkt_fused_workspace_bytes)");
    if (!taker) return refuse(MPC_E_DIMS, nobody, nobody_is_no_kernel);
    r.kernel = taker->code;
    return r;
}

// Which fused kernel takes this backward.  Launches nothing, sets no error state, allocates nothing; never cached.  The refusals
// are mpc_lqr_kkt_fused's, in its order (behind check_kkt_fused); no_kernel marks the two that say "legal, but no fused kernel".
KktRoute kkt_fused_route(const StepParams<float> &sp, const mpc_lqr_problem *p, const KktPointers &a, int64_t workspace_bytes)
{
    KktRoute r = {0, nullptr, false, MPC_KKT_NONE, 0};
    const auto refuse = [&r](int code, const char *msg, bool no_kernel = false) { r.code = code; r.msg = msg; r.no_kernel = no_kernel; return r; };
    // A kernel that takes the views takes their sizes, so the call that somebody takes asks every rule at most once.  Only the call
    // nobody takes asks a second time, on the sizes alone, for the kernel it was heading for: that one names the workspace and the text.
    const KktKernel *const taker = kkt_first(p, sp, a), *const heading = taker ? taker : kkt_first(p, sp, a, true);
    if (!heading)
        return refuse(MPC_E_DIMS, "mpc_lqr_kkt_fused: needs fp32, n_state <= 32, n_ctrl <= 8, and "
                                  "MPC_OPT_C_SYMMETRIC (otherwise: mpc_lqr_kkt_prepare + mpc_lqr_step + mpc_lqr_kkt_grads)", true);
    return kkt_route_shared(p, a, workspace_bytes, taker, heading, heading->nobody, true);
}

// "<entry>: <kernel> needs <what>" for a call that names a kernel (thread-local: the text outlives the route that points at it)
static const char *kkt_named_refusal(const KktKernel &k, const char *what)
{
    static thread_local std::string text;
    text = std::string("mpc_lqr_kkt_fused_kernel: ") + k.name + " needs " + what;
    return text.c_str();
}

// The same decision for a call that asks for a kernel (mpc_lqr_kkt_fused_kernel): 0 = nobody asked, kkt_fused_route itself; an exact
// MPC_KKT_* code = that kernel or a refusal that names it and the first thing it misses (never "no kernel": the caller asked for one);
// MPC_KKT_PREFER_NARROW = the one-tile kernels, 16-byte gathers first, where they take the call and no 12/4-family kernel takes its
// sizes -- those are faster up to 12/4 -- and the order of kernel = 0 everywhere else.
KktRoute kkt_fused_route_kernel(const StepParams<float> &sp, const mpc_lqr_problem *p, const KktPointers &a, int64_t workspace_bytes, int kernel)
{
    if (kernel == MPC_KKT_NONE) return kkt_fused_route(sp, p, a, workspace_bytes);
    KktRoute r = {0, nullptr, false, MPC_KKT_NONE, 0};
    const auto refuse = [&r](int code, const char *msg) { r.code = code; r.msg = msg; return r; };
    const auto row = [](int code) { return &kkt_order[code - 1]; };
    const bool f32 = p->dtype == MPC_F32;
    if (kernel == MPC_KKT_PREFER_NARROW) {
        const KktKernel *taker = nullptr;
        if (!f32 || kkt_kernel_takes(MPC_KKT_DPP16, sp, a, true) || kkt_kernel_takes(MPC_KKT_DPP16_PAD, sp, a, true) ||
            !kkt_kernel_takes(MPC_KKT_MFMA40_NARROW4, sp, a, true))
            return kkt_fused_route(sp, p, a, workspace_bytes);
        // (a view the dword kernel refuses -- the workspace, tensor bounds -- the two-tile kernels refuse as well: nobody takes it)
        for (int code : {MPC_KKT_MFMA40_NARROW16, MPC_KKT_MFMA40_NARROW4})
            if (!taker && kkt_kernel_takes(code, sp, a)) taker = row(code);
        return kkt_route_shared(p, a, workspace_bytes, taker, taker ? taker : row(MPC_KKT_MFMA40_NARROW4), kkt_nobody_narrow, true);
    }
    if (kernel < 1 || kernel > (int)(sizeof(kkt_order) / sizeof(kkt_order[0])))
        return refuse(MPC_E_ARG, "mpc_lqr_kkt_fused_kernel: unknown kernel code (MPC_KKT_*)");
    const KktKernel &k = *row(kernel);
    if (!f32) return refuse(MPC_E_DIMS, kkt_named_refusal(k, "float32"));
    if (!sp.c_symmetric) return refuse(MPC_E_DIMS, kkt_named_refusal(k, "MPC_OPT_C_SYMMETRIC"));
    if (sp.env.kind) return refuse(MPC_E_DIMS, kkt_named_refusal(k, "a linear model (no simulator)"));
    if (!kkt_kernel_takes(kernel, sp, a, true)) return refuse(MPC_E_DIMS, kkt_named_refusal(k, k.sizes));
    return kkt_route_shared(p, a, workspace_bytes, kkt_kernel_takes(kernel, sp, a) ? &k : nullptr, &k, kkt_named_refusal(k, k.views), false);
}

// the argument checks of mpc_lqr_kkt_fused, and of mpc_lqr_kkt_fused_route, which answers for the same arguments
static int check_kkt_fused(const mpc_lqr_problem *p, const mpc_lqr_options *o)
{
    const int rc = check_problem(p, true, true);
    return rc ? rc : check_options(p, o);
}

static StepParams<float> kkt_fused_params(const mpc_lqr_problem *p, const mpc_lqr_options *o, int32_t *status)
{
    mpc_lqr_outputs out;
    memset(&out, 0, sizeof(out));
    out.status = status;
    return make_params<float>(p, o, &out);
}

// Which kernel takes the closed-form part of the three-call route (mpc_lqr_kkt_grads): the first of this order that takes the views.
static int kkt_grads_route(const StepParams<float> &sp, const float *dx, const float *du, const float *dl_dx, const float *dC, const float *dF)
{
    // headline shape: the 4-problems-per-wave DPP kernel (lqr_dpp16_body.h: kkt_wave)
    if (kkt_dpp16_supported(sp, dx, du, dl_dx, dC, dF)) return MPC_KKT_GRADS_DPP16;
    // other shapes up to n = 64: costate recursion per wavefront + fully parallel outer products
    if (kkt_wave_supported(sp, dx, du, dl_dx, dC, dF)) return MPC_KKT_GRADS_WAVE;
    return MPC_KKT_GRADS_GENERIC;
}

// the argument checks of mpc_lqr_kkt_grads and mpc_lqr_kkt_grads_route (an empty batch passes them: nothing is launched)
static int check_kkt_grads(const mpc_lqr_problem *p, const void *dx, const void *du, const void *dl_dx, const void *dl_du, const void *dC,
                           const void *dc, const void *dF, const void *dx_init)
{
    const int rc = check_problem(p, true, true);
    if (rc || p->B == 0) return rc;
    if (!dx || !du || !dl_dx || !dl_du || !dC || !dc || !dx_init) return fail(MPC_E_NULL, "kkt_grads: NULL argument");
    if (p->T > 1 && !dF) return fail(MPC_E_NULL, "kkt_grads: dF is NULL");
    return MPC_OK;
}
}  // namespace mpclqr

using namespace mpclqr;

// The argument checks of mpc_mlp_rollout and mpc_mlp_rollout_dtype behind their NULL / size / dtype tests, written once for both
// reals; fills `sp`.  `empty`: B = 0, nothing to launch.
template <typename real>
static int mlp_rollout_params(const mpc_lqr_problem *p, const mpc_lqr_options *o, const void *K, const void *k, const void *old_costs,
                              const mpc_lqr_outputs *out, StepParams<real> &sp, bool &empty)
{
    empty = p->B == 0;
    if (empty) return MPC_OK;
    if (!p->x_init || !p->cur_u) return fail(MPC_E_NULL, "x_init / current_u is NULL");
    if ((p->C == nullptr) != (p->c == nullptr)) return fail(MPC_E_NULL, "pass both C and c, or neither");
    if (!out->new_x) return fail(MPC_E_NULL, "new_x is NULL");
    if ((K == nullptr) != (k == nullptr)) return fail(MPC_E_NULL, both_gains);
    if (K) {
        if (!p->cur_x || !p->C || !old_costs || !out->new_u)
            return fail(MPC_E_NULL, "line search needs current_x, C, c, old_costs and new_u");
        int rc = check_options(p, o);
        if (rc) return rc;
        if (o && o->true_dynamics) return fail(MPC_E_ARG, "mpc_mlp_rollout: options.true_dynamics must be NULL");
    }
    sp = make_params<real>(p, K ? o : nullptr, out);
    sp.K = (real *)K;
    sp.k = (real *)k;
    sp.old_costs_in = (const real *)old_costs;
    return MPC_OK;
}

extern "C" {

int mpc_lqr_abi_version(void) { return MPC_LQR_ABI_VERSION; }

const char *mpc_lqr_build_info(void)
{
    return "libmpc_lqr_hip gfx950 (CDNA4) | kernels: lqr_step_generic<f32,f64>, lqr_step_mfma16<f32,f64>, lqr_step_dpp16<f32>, lqr_step_dpp16_padded<f32>, "
           "lqr_step_tiny<f32,f64>, lqr_step_wave1<f32>, lqr_step_wave1_carry<f32>, lqr_step_mfma40<f32>, lqr_step_mfma40_padded<f32>, lqr_step_mfma40_narrow<f32>, nn_rollout<f32,f64>, nn_linearize<f32,f64>, nn_param_grad<f32>, nn_param_grad64, env_linearize, env_param_grad<f32,f64>, kkt_grads, kkt_grads_shared<f32>, kkt_fused<f32>, kkt_fused_padded<f32>, kkt_fused_narrow<f32>, pnqp, traj_cost, select_best, slew_augment<f32,f64>, kkt_grads_wave<f64> | built " __DATE__ " " __TIME__;
}

const char *mpc_lqr_last_error(void) { return g_last_error.c_str(); }

int64_t mpc_lqr_workspace_bytes(const mpc_lqr_problem *p)
{
    if (!p) return 0;
    // + one status word per problem for callers that pass out->status = NULL (see step_impl)
    return status_scratch_offset(p) + (int64_t)p->B * 4 + 256;
}

int mpc_lqr_step(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_lqr_outputs *out,
                 void *workspace, int64_t workspace_bytes, int impl, void *stream)
{
    const int rc = check_step(p, o, out);
    if (rc) return rc;
    if (p->B == 0) return MPC_OK;
    hipStream_t st = (hipStream_t)stream;
    return p->dtype == MPC_F32 ? step_impl<float>(p, o, out, workspace, workspace_bytes, impl, 3, nullptr, st)
                               : step_impl<double>(p, o, out, workspace, workspace_bytes, impl, 3, nullptr, st);
}

int64_t mpc_lqr_resident_launches(void) { return g_resident_launches.load(std::memory_order_relaxed); }

int mpc_lqr_step_route(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_lqr_outputs *out, const void *workspace,
                       int64_t workspace_bytes, int impl, int *ring)
{
    const int rc = check_step(p, o, out);
    if (rc) return rc;
    if (ring) *ring = 0;
    if (p->B == 0) return 0;                 // (mpc_lqr_step succeeds and launches nothing)
    return p->dtype == MPC_F32 ? route_query<float>(p, o, out, workspace, workspace_bytes, impl, ring)
                               : route_query<double>(p, o, out, workspace, workspace_bytes, impl, ring);
}

int mpc_lqr_impl_supported(const mpc_lqr_problem *p, const mpc_lqr_options *o, int impl)
{
    if (!p || check_problem(p, false, false) != MPC_OK || check_options(p, o) != MPC_OK) return 0;
    if (!known_kernel(impl)) return 0;
    const StepKernel &k = step_kernels[impl];
    // (MPC_ENV_CTRL_CARRY: the kernels that carry the control, see step_route)
    if (o && o->true_dynamics && (o->true_dynamics->kind & MPC_ENV_CTRL_CARRY) && !(k.flags & K_CARRIES)) return 0;
    if ((k.flags & K_CARRY_ONLY) && o && (o->flags & MPC_OPT_SWEEP_ONLY)) return 0;          // (a whole step only)
    // sizes, dtype and options -- and, for the kernels that stream 16-byte granules (3, 5), the alignment of the blocks p names: the
    // answer mpc_lqr_step gives a forced call for the same reason.  (Workspace and outputs are the call's: checked there.)
    return p->dtype == MPC_F32 ? kernel_takes<float>(k, make_params<float>(p, o, nullptr), true)
                               : kernel_takes<double>(k, make_params<double>(p, o, nullptr), true);
}

int mpc_lqr_row_carry_pays(const mpc_lqr_problem *p, const mpc_lqr_options *o)
{
    // (silent: what the argument checks say about a call impl 10 would refuse is not left behind)
    const std::string keep = g_last_error;
    // (sizes, dtype and options, as mpc_lqr_impl_supported -- but F may be NULL at any T: a linearising simulator has none)
    const bool pays = p && o && check_problem(p, false, false, false) == MPC_OK && check_options(p, o) == MPC_OK && p->B > 0 &&
                      p->dtype == MPC_F32 && !(o->flags & MPC_OPT_SWEEP_ONLY) && wave1_carry_pays(make_params<float>(p, o, nullptr));
    g_last_error = keep;
    return pays ? 1 : 0;
}

int mpc_lqr_qp_record(const mpc_lqr_problem *p, const mpc_lqr_options *o, int impl, int64_t *offset_bytes, int64_t *st, int64_t *sb)
{
    // the route of a box-constrained float32 step whose out->K / out->k are NULL, on a workspace of mpc_lqr_workspace_bytes
    if (!p || !o || !offset_bytes || !st || !sb) return 0;
    if (check_problem(p, false, false) != MPC_OK || check_options(p, o) != MPC_OK) return 0;
    if (p->dtype != MPC_F32 || o->bound_mode == MPC_BOUND_NONE || o->true_dynamics || p->B == 0) return 0;
    mpc_lqr_outputs out;
    memset(&out, 0, sizeof(out));
    out.new_x = out.new_u = (void *)16;          // (a step has them; the route looks at pointers for NULL and alignment only)
    // (a forced impl 5 has always been answered from the sizes alone: off the 16-byte grid the step itself is refused at launch)
    const bool by_sizes = known_kernel(impl) && (step_kernels[impl].flags & K_SIZES_RECORD);
    const mpc_lqr_problem q = by_sizes ? sizes_only(p->B, p->T, p->ns, p->nc, p->dtype) : *p;
    const StepParams<float> sp = make_params<float>(&q, o, &out);
    const StepRoute r = step_route(sp, p, impl, 3, (const void *)16, mpc_lqr_workspace_bytes(p));
    if (r.code || r.qp_off < 0) return 0;        // 0 = not filled (only where the kernel that keeps the record really takes the call)
    *offset_bytes = r.qp_off; *st = r.qp_st; *sb = r.qp_sb;
    return 1;
}

int mpc_lqr_sweep(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_lqr_outputs *out, void *stream)
{
    return sweep_or_rollout(p, o, out, 1, nullptr, stream);
}

int mpc_lqr_rollout(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_lqr_outputs *out,
                    const void *old_costs_in, void *stream)
{
    return sweep_or_rollout(p, o, out, 2, old_costs_in, stream);
}

int mpc_lqr_kkt_grads(const mpc_lqr_problem *p, const void *dx_, const void *du_, const void *dl_dx_,
                      const void *dl_du, void *dC_, void *dc_, void *dF_, void *df_, void *dx_init_, void *stream)
{
    const int rc = check_kkt_grads(p, dx_, du_, dl_dx_, dl_du, dC_, dc_, dF_, dx_init_);
    if (rc || p->B == 0) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p->dtype != MPC_F32)                     // float64: always the generic kernel
        return launch_kkt_grads<double>(make_params<double>(p, nullptr, nullptr), (const double *)dx_, (const double *)du_,
                                        (const double *)dl_dx_, (const double *)dl_du, (double *)dC_, (double *)dc_, (double *)dF_,
                                        (double *)df_, (double *)dx_init_, st);
    const StepParams<float> sp = make_params<float>(p, nullptr, nullptr);
    const float *dx = (const float *)dx_, *du = (const float *)du_, *dl_dx = (const float *)dl_dx_;
    float *dC = (float *)dC_, *dc = (float *)dc_, *dF = (float *)dF_, *df = (float *)df_, *dx_init = (float *)dx_init_;
    switch (kkt_grads_route(sp, dx, du, dl_dx, dC, dF)) {
    case MPC_KKT_GRADS_DPP16: return launch_kkt_dpp16(sp, dx, du, dl_dx, dC, dc, dF, df, dx_init, st);
    case MPC_KKT_GRADS_WAVE: return launch_kkt_wave(sp, dx, du, dl_dx, dC, dc, dF, df, dx_init, st);
    }
    return launch_kkt_grads<float>(sp, dx, du, dl_dx, (const float *)dl_du, dC, dc, dF, df, dx_init, st);
}

int mpc_lqr_kkt_grads_route(const mpc_lqr_problem *p, const void *dx, const void *du, const void *dl_dx, const void *dl_du,
                            const void *dC, const void *dc, const void *dF, const void *df, const void *dx_init)
{
    const int rc = check_kkt_grads(p, dx, du, dl_dx, dl_du, dC, dc, dF, dx_init);
    if (rc || p->B == 0) return rc;          // (0: mpc_lqr_kkt_grads succeeds and launches nothing)
    if (p->dtype != MPC_F32) return MPC_KKT_GRADS_GENERIC;
    return kkt_grads_route(make_params<float>(p, nullptr, nullptr), (const float *)dx, (const float *)du, (const float *)dl_dx,
                           (const float *)dC, (const float *)dF);
}

// (4) with the kernel named by the caller.  MPC_KKT_GRADS_WAVE64 is the one code there is: the float64 wavefront kernels
// (kkt_wave64.hip), which kernel = 0 never picks -- float64 stays on the generic kernel there, the recorded routes stay.
int mpc_lqr_kkt_grads_kernel_supported(const mpc_lqr_problem *p, int kernel)
{
    if (!p || kernel != MPC_KKT_GRADS_WAVE64 || p->B < 0 || p->T < 1 || p->ns < 1 || p->nc < 1) return 0;
    return (p->dtype == MPC_F64 && kkt_wave64_sizes(p->ns, p->nc)) ? 1 : 0;
}

int mpc_lqr_kkt_grads_kernel_route(const mpc_lqr_problem *p, int kernel, const void *dx, const void *du, const void *dl_dx,
                                   const void *dl_du, const void *dC, const void *dc, const void *dF, const void *df, const void *dx_init)
{
    if (kernel == 0) return mpc_lqr_kkt_grads_route(p, dx, du, dl_dx, dl_du, dC, dc, dF, df, dx_init);
    const int rc = check_kkt_grads(p, dx, du, dl_dx, dl_du, dC, dc, dF, dx_init);
    if (rc) return rc;
    if (kernel != MPC_KKT_GRADS_WAVE64) return fail(MPC_E_ARG, "mpc_lqr_kkt_grads_kernel: unknown kernel code (MPC_KKT_GRADS_WAVE64)");
    if (p->B == 0) return 0;                 // (mpc_lqr_kkt_grads_kernel succeeds and launches nothing)
    // the kernel's own refusals, the first thing it misses.  (A linear model: this entry carries no options, so no simulator can be
    // named to it -- F is the model, and check_kkt_grads has asked for it.)
    if (p->dtype != MPC_F64) return fail(MPC_E_DIMS, "mpc_lqr_kkt_grads_kernel: MPC_KKT_GRADS_WAVE64 needs float64");
    if (!kkt_wave64_sizes(p->ns, p->nc))
        return fail(MPC_E_DIMS, "mpc_lqr_kkt_grads_kernel: MPC_KKT_GRADS_WAVE64 needs 2 <= n_state + n_ctrl <= 64");
    uintptr_t bits = 0;
    for (const void *q : {p->C, p->c, p->F, p->cur_x, p->cur_u, dx, du, dl_dx, dC, dc, dF, df, dx_init}) bits |= (uintptr_t)q;
    if (bits & 7) return fail(MPC_E_DIMS, "mpc_lqr_kkt_grads_kernel: MPC_KKT_GRADS_WAVE64 needs every pointer 8-byte aligned");
    return MPC_KKT_GRADS_WAVE64;
}

int mpc_lqr_kkt_grads_kernel(const mpc_lqr_problem *p, int kernel, const void *dx, const void *du, const void *dl_dx,
                             const void *dl_du, void *dC, void *dc, void *dF, void *df, void *dx_init, void *stream)
{
    if (kernel == 0) return mpc_lqr_kkt_grads(p, dx, du, dl_dx, dl_du, dC, dc, dF, df, dx_init, stream);
    const int route = mpc_lqr_kkt_grads_kernel_route(p, kernel, dx, du, dl_dx, dl_du, dC, dc, dF, df, dx_init);
    if (route <= 0) return route;            // (a refusal, or B = 0: nothing is launched)
    return launch_kkt_wave64(make_params<double>(p, nullptr, nullptr), (const double *)dx, (const double *)du, (const double *)dl_dx,
                             (double *)dC, (double *)dc, (double *)dF, (double *)df, (double *)dx_init, (hipStream_t)stream);
}

int mpc_lqr_kkt_shared_supported(const mpc_lqr_problem *p)
{
    if (!p || p->B < 0 || p->T < 1 || p->ns < 1 || p->nc < 1) return 0;
    return (p->dtype == MPC_F32 && p->ns + p->nc <= 64) ? 1 : 0;
}

int64_t mpc_lqr_kkt_shared_workspace_bytes(const mpc_lqr_problem *p)
{
    if (!mpc_lqr_kkt_shared_supported(p)) return 0;
    return kkt_shared_workspace_bytes(p->T, p->B, p->ns, p->nc);
}

int mpc_lqr_kkt_grads_shared(const mpc_lqr_problem *p, const void *dx, const void *du, const void *dl_dx, const void *dl_du,
                             void *sum_dC, void *sum_dc, void *sum_dF, void *sum_df, void *dx_init, void *workspace,
                             int64_t workspace_bytes, void *stream)
{
    int rc = check_problem(p, true, true);
    if (rc) return rc;
    if (!mpc_lqr_kkt_shared_supported(p))
        return fail(MPC_E_DIMS, "mpc_lqr_kkt_grads_shared: needs float32 and n_state + n_ctrl <= 64 (otherwise: mpc_lqr_kkt_grads and a sum over the batch)");
    if (p->B == 0) return MPC_OK;
    if (!dx || !du || !dl_dx || !dl_du || !dx_init) return fail(MPC_E_NULL, "kkt_grads_shared: NULL argument");
    if (!workspace) return fail(MPC_E_NULL, "kkt_grads_shared: the workspace is NULL");
    if (workspace_bytes < mpc_lqr_kkt_shared_workspace_bytes(p))
        return fail(MPC_E_DIMS, "workspace too small (see mpc_lqr_kkt_shared_workspace_bytes)");
    if ((uintptr_t)workspace % 16) return fail(MPC_E_ARG, "kkt_grads_shared: the workspace must be 16-byte aligned");
    StepParams<float> sp = make_params<float>(p, nullptr, nullptr);
    return launch_kkt_shared(sp, (const float *)dx, (const float *)du, (const float *)dl_dx, (float *)sum_dC, (float *)sum_dc,
                             p->T > 1 ? (float *)sum_dF : nullptr, p->T > 1 ? (float *)sum_df : nullptr, (float *)dx_init, workspace,
                             (hipStream_t)stream);
}

int mpc_lqr_kkt_fused_supported(const mpc_lqr_problem *p, const mpc_lqr_options *o)
{
    if (!p || check_problem(p, false, false) != MPC_OK || check_options(p, o) != MPC_OK) return 0;
    // (12/4: any horizon since round 4; every shape UP TO 12/4 since round 6: the padded instantiation, lqr_dpp16.hip -DMPC_DPP16_PAD_KKT)
    // ... and every shape up to 32/8: the padded instantiation of the 32/8 kernel's fused backward, lqr_mfma40.hip -DMPC_MFMA40_KKT -DMPC_MFMA40_PAD=4
    return kkt_first(p, make_params<float>(p, o, nullptr), KktPointers(), true) ? 1 : 0;
}

int64_t mpc_lqr_kkt_fused_workspace_bytes(const mpc_lqr_problem *p)
{
    if (!p) return 0;
    // The workspace of the kernel a float32 backward of these sizes heads for under MPC_OPT_C_SYMMETRIC; where there is none (a larger
    // shape) the last of the order answers, and sizes below 1, which every entry refuses, answer as 1 does -- as they always have.
    const mpc_lqr_problem q = sizes_only(1, 1, std::max(p->ns, 1), std::max(p->nc, 1), MPC_F32);
    StepParams<float> s = make_params<float>(&q, nullptr, nullptr);
    s.c_symmetric = 1;
    const KktKernel *heading = kkt_first(&q, s, KktPointers(), true);
    return (heading ? heading : &kkt_order[MPC_KKT_MFMA40_PAD4 - 1])->ws_bytes(p->T, p->B);
}

int64_t mpc_lqr_kkt_fused_kernel_workspace_bytes(const mpc_lqr_problem *p, const mpc_lqr_options *o, int kernel)
{
    if (!p) return 0;
    if (kernel >= 1 && kernel <= (int)(sizeof(kkt_order) / sizeof(kkt_order[0]))) return kkt_order[kernel - 1].ws_bytes(p->T, p->B);
    if (kernel == MPC_KKT_PREFER_NARROW && p->dtype == MPC_F32 && check_problem(p, false, false) == MPC_OK && check_options(p, o) == MPC_OK) {
        // where the family rule of kkt_fused_route_kernel heads for a one-tile kernel: sizes, dtype and flags (no options: as vouched)
        StepParams<float> s = make_params<float>(p, o, nullptr);
        if (!o) s.c_symmetric = 1;
        if (!kkt_kernel_takes(MPC_KKT_DPP16, s, KktPointers(), true) && !kkt_kernel_takes(MPC_KKT_DPP16_PAD, s, KktPointers(), true) &&
            kkt_kernel_takes(MPC_KKT_MFMA40_NARROW4, s, KktPointers(), true))
            return kkt_order[MPC_KKT_MFMA40_NARROW4 - 1].ws_bytes(p->T, p->B);
    }
    return kernel == MPC_KKT_NONE || kernel == MPC_KKT_PREFER_NARROW ? mpc_lqr_kkt_fused_workspace_bytes(p) : 0;
}

int mpc_lqr_kkt_fused(const mpc_lqr_problem *p, const mpc_lqr_options *o, const void *dl_dx, const void *dl_du,
                      void *dC, void *dc, void *dF, void *df, void *dx_init, void *dx_out, void *du_out, int32_t *status,
                      void *workspace, int64_t workspace_bytes, void *stream)
{
    return mpc_lqr_kkt_fused_kernel(p, o, MPC_KKT_NONE, dl_dx, dl_du, dC, dc, dF, df, dx_init, dx_out, du_out, status, workspace, workspace_bytes, stream);
}

int mpc_lqr_kkt_fused_route(const mpc_lqr_problem *p, const mpc_lqr_options *o, const void *dl_dx, const void *dl_du,
                            const void *dC, const void *dc, const void *dF, const void *df, const void *dx_init, const void *dx_out,
                            const void *du_out, const int32_t *status, const void *workspace, int64_t workspace_bytes)
{
    return mpc_lqr_kkt_fused_kernel_route(p, o, MPC_KKT_NONE, dl_dx, dl_du, dC, dc, dF, df, dx_init, dx_out, du_out, status, workspace, workspace_bytes);
}

int mpc_lqr_kkt_fused_kernel(const mpc_lqr_problem *p, const mpc_lqr_options *o, int kernel, const void *dl_dx, const void *dl_du,
                             void *dC, void *dc, void *dF, void *df, void *dx_init, void *dx_out, void *du_out, int32_t *status,
                             void *workspace, int64_t workspace_bytes, void *stream)
{
    // (MPC_KKT_NONE: nobody asked -- kkt_fused_route_kernel is kkt_fused_route then, and this is mpc_lqr_kkt_fused)
    const int rc = check_kkt_fused(p, o);
    if (rc) return rc;
    const StepParams<float> sp = kkt_fused_params(p, o, status);
    const KktRoute r = kkt_fused_route_kernel(sp, p, KktPointers{dl_dx, dl_du, dC, dc, dF, df, dx_init, dx_out, du_out, workspace},
                                              workspace_bytes, kernel);
    if (r.code) return fail(r.code, r.msg);
    if (!r.kernel) return MPC_OK;                // (an empty batch)
    // the nested solve is a plain LQRStep(...) in the reference (:328-338): linesearch_decay 0.2, max_linesearch_iter 10
    return kkt_order[r.kernel - 1].launch(sp, (const float *)dl_dx, (const float *)dl_du, (float *)dC, (float *)dc, (float *)dF, (float *)df,
                                          (float *)dx_init, (float *)dx_out, (float *)du_out, (float *)workspace, 0.2f, 10, (hipStream_t)stream);
}

int mpc_lqr_kkt_fused_kernel_route(const mpc_lqr_problem *p, const mpc_lqr_options *o, int kernel, const void *dl_dx, const void *dl_du,
                                   const void *dC, const void *dc, const void *dF, const void *df, const void *dx_init, const void *dx_out,
                                   const void *du_out, const int32_t *status, const void *workspace, int64_t workspace_bytes)
{
    const int rc = check_kkt_fused(p, o);
    if (rc) return rc;
    const KktRoute r = kkt_fused_route_kernel(kkt_fused_params(p, o, (int32_t *)status), p,
                                              KktPointers{dl_dx, dl_du, dC, dc, dF, df, dx_init, dx_out, du_out, workspace}, workspace_bytes, kernel);
    if (r.code && !r.no_kernel) return fail(r.code, r.msg);
    return r.kernel;                             // (MPC_KKT_NONE: a legal call that no fused kernel takes, or an empty batch)
}

int mpc_env_traj_cost(const mpc_lqr_problem *p, const mpc_env_dynamics *env, void *x, void *cost, void *stream)
{
    if (!p || !env) return fail(MPC_E_NULL, "problem / simulator is NULL");
    if (p->B < 0 || p->T < 1) return fail(MPC_E_DIMS, "need B>=0, T>=1");
    if (p->dtype != MPC_F32 && p->dtype != MPC_F64) return fail(MPC_E_DTYPE, "dtype must be MPC_F32 or MPC_F64");
    int rc = check_env(env, p->ns, p->nc);
    if (rc) return rc;
    if (p->B == 0) return MPC_OK;
    if (!p->x_init || !p->cur_u) return fail(MPC_E_NULL, "x_init / u is NULL");
    if (cost && (!p->C || !p->c)) return fail(MPC_E_NULL, "cost requested but C / c is NULL");
    return by_dtype(p->dtype, [&](auto t) {
        typedef decltype(t) real;
        StepParams<real> sp = make_params<real>(p, nullptr, nullptr);
        set_env(sp.env, env);
        return launch_traj_cost<real>(sp, (real *)x, (real *)cost, (hipStream_t)stream);
    });
}

int mpc_slew_augment(const mpc_lqr_problem *p, double gamma, void *aC, void *ac, void *aF, void *af, void *stream)
{
    if (!p) return fail(MPC_E_NULL, "problem is NULL");
    if (p->B < 0 || p->T < 1 || p->ns < 1 || p->nc < 1) return fail(MPC_E_DIMS, "need B>=0, T>=1, ns>=1, nc>=1");
    if (p->dtype != MPC_F32 && p->dtype != MPC_F64) return fail(MPC_E_DTYPE, "dtype must be MPC_F32 or MPC_F64");
    if (p->B == 0) return MPC_OK;
    if (!p->C || !p->c || !aC || !ac) return fail(MPC_E_ARG, "slew_augment: C / c / aC / ac is NULL");
    // (F NULL: a simulator behind MPC_ENV_CTRL_CARRY has no F, f -- only the cost is augmented)
    if (p->T > 1 && ((p->F == nullptr) != (aF == nullptr))) return fail(MPC_E_ARG, "slew_augment: F and aF go together");
    if (p->T > 1 && p->f && (!af || !p->F)) return fail(MPC_E_ARG, "slew_augment: f given but af / F is NULL");
    if (p->C_st < 0 || p->C_sb < 0 || p->c_st < 0 || p->c_sb < 0 || p->F_st < 0 || p->F_sb < 0 || p->f_st < 0 || p->f_sb < 0)
        return fail(MPC_E_ARG, "slew_augment: negative stride");
    hipStream_t st = (hipStream_t)stream;
    return p->dtype == MPC_F32 ? launch_slew_augment<float>(p, gamma, (float *)aC, (float *)ac, (float *)aF, (float *)af, st)
                               : launch_slew_augment<double>(p, gamma, (double *)aC, (double *)ac, (double *)aF, (double *)af, st);
}

int mpc_env_linearize(const mpc_env_dynamics *env, int dtype, int64_t N, const void *x, const void *u, void *F,
                      void *f, void *stream)
{
    const int rc = check_env_points(env, dtype, N);
    if (rc || N == 0) return rc;
    if (!x || !u || !F || !f) return fail(MPC_E_NULL, "env_linearize: NULL argument");
    return by_dtype(dtype, [&](auto t) {
        typedef decltype(t) real;
        EnvDesc<real> e;
        set_env(e, env);
        return launch_env_linearize<real>(e, (long)N, (const real *)x, (const real *)u, (real *)F, (real *)f, (hipStream_t)stream);
    });
}

int64_t mpc_env_param_grad_workspace_bytes(int64_t N) { return env_param_grad_workspace_bytes(N < 0 ? 0 : N); }

int mpc_env_param_grad(const mpc_env_dynamics *env, int dtype, int64_t N, const void *x, const void *u, const void *gF,
                       const void *gf, void *gparams, void *workspace, int64_t workspace_bytes, void *stream)
{
    const int rc = check_env_points(env, dtype, N);
    if (rc || N == 0) return rc;
    if (!x || !u || !gF || !gf || !gparams || !workspace) return fail(MPC_E_NULL, "env_param_grad: NULL argument");
    if (workspace_bytes < env_param_grad_workspace_bytes(N))
        return fail(MPC_E_DIMS, "workspace too small (see mpc_env_param_grad_workspace_bytes)");
    if ((uintptr_t)workspace % 8) return fail(MPC_E_ARG, "env_param_grad: the workspace must be 8-byte aligned");
    return by_dtype(dtype, [&](auto t) {
        typedef decltype(t) real;
        EnvDesc<real> e;
        set_env(e, env);
        return launch_env_param_grad<real>(e, (long)N, (const real *)x, (const real *)u, (const real *)gF, (const real *)gf, (real *)gparams,
                                           (double *)workspace, (hipStream_t)stream);
    });
}

int64_t mpc_mlp_workspace_bytes(const mpc_mlp_dynamics *net) { return nn_workspace_bytes(net); }

int mpc_mlp_supported(const mpc_mlp_dynamics *net, int n_state, int n_ctrl) { return nn_budget(net, n_state, n_ctrl); }

int mpc_mlp_rollout(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_mlp_dynamics *net, const void *K,
                    const void *k, const void *old_costs, const mpc_lqr_outputs *out, void *workspace,
                    int64_t workspace_bytes, void *stream)
{
    if (!p || !out) return fail(MPC_E_NULL, "problem / outputs is NULL");
    if (p->B < 0 || p->T < 1 || p->ns < 1 || p->nc < 1) return fail(MPC_E_DIMS, "need B>=0, T>=1, ns>=1, nc>=1");
    if (p->dtype != MPC_F32) return fail(MPC_E_DTYPE, "the network kernels are fp32 only");
    StepParams<float> sp;
    bool empty;
    const int rc = mlp_rollout_params<float>(p, o, K, k, old_costs, out, sp, empty);
    if (rc || empty) return rc;
    return launch_nn_rollout(sp, net, workspace, workspace_bytes, (hipStream_t)stream);
}

int mpc_mlp_linearize(const mpc_mlp_dynamics *net, int n_state, int n_ctrl, int64_t N, const void *x, const void *u,
                      void *F, void *f, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (n_state < 1 || n_ctrl < 1 || N < 0) return fail(MPC_E_DIMS, "need n_state>=1, n_ctrl>=1, N>=0");
    if (N == 0) return MPC_OK;
    if (!x || !u || !F || !f) return fail(MPC_E_NULL, "mlp_linearize: NULL argument");
    return launch_nn_linearize(net, (long)N, n_state, n_ctrl, (const float *)x, (const float *)u, (float *)F, (float *)f,
                               workspace, workspace_bytes, (hipStream_t)stream);
}

int mpc_mlp_linearize_carry(const mpc_mlp_dynamics *net, int n_state, int n_ctrl, int64_t N, const void *z, const void *u,
                            void *aF, void *af, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (n_state < 1 || n_ctrl < 1 || N < 0) return fail(MPC_E_DIMS, "need n_state>=1, n_ctrl>=1, N>=0");
    if (n_state + n_ctrl > 32) return fail(MPC_E_DIMS, "mlp_linearize_carry: n_state + n_ctrl <= 32 (the augmented state of the step kernels)");
    if (N == 0) return MPC_OK;
    if (!z || !u || !aF || !af) return fail(MPC_E_NULL, "mlp_linearize_carry: NULL argument");
    return launch_nn_linearize_carry(net, (long)N, n_state, n_ctrl, (const float *)z, (const float *)u, (float *)aF, (float *)af,
                                     workspace, workspace_bytes, (hipStream_t)stream);
}

// (6d') the entries above with a dtype: MPC_F32 is the entry above itself, MPC_F64 the plain-FMA kernels of nn_dynamics64.hip
int mpc_mlp_supported_dtype(const mpc_mlp_dynamics *net, int n_state, int n_ctrl, int dtype)
{
    return dtype == MPC_F32 ? nn_budget(net, n_state, n_ctrl) : (dtype == MPC_F64 ? nn64_budget(net, n_state, n_ctrl) : 0);
}

int64_t mpc_mlp_workspace_bytes_dtype(const mpc_mlp_dynamics *net, int dtype)
{
    return dtype == MPC_F32 ? nn_workspace_bytes(net) : (dtype == MPC_F64 ? nn64_workspace_bytes(net) : 0);
}

int mpc_mlp_rollout_dtype(const mpc_lqr_problem *p, const mpc_lqr_options *o, const mpc_mlp_dynamics *net, const void *K,
                          const void *k, const void *old_costs, const mpc_lqr_outputs *out, void *workspace,
                          int64_t workspace_bytes, void *stream)
{
    if (!p || !out) return fail(MPC_E_NULL, "problem / outputs is NULL");
    if (p->dtype == MPC_F32) return mpc_mlp_rollout(p, o, net, K, k, old_costs, out, workspace, workspace_bytes, stream);
    if (p->B < 0 || p->T < 1 || p->ns < 1 || p->nc < 1) return fail(MPC_E_DIMS, "need B>=0, T>=1, ns>=1, nc>=1");
    if (p->dtype != MPC_F64) return fail(MPC_E_DTYPE, "bad dtype");
    StepParams<double> sp;
    bool empty;
    const int rc = mlp_rollout_params<double>(p, o, K, k, old_costs, out, sp, empty);
    if (rc || empty) return rc;
    return launch_nn64_rollout(sp, net, workspace, workspace_bytes, (hipStream_t)stream);
}

int mpc_mlp_linearize_dtype(const mpc_mlp_dynamics *net, int dtype, int n_state, int n_ctrl, int64_t N, const void *x, const void *u,
                            void *F, void *f, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (dtype == MPC_F32) return mpc_mlp_linearize(net, n_state, n_ctrl, N, x, u, F, f, workspace, workspace_bytes, stream);
    if (dtype != MPC_F64) return fail(MPC_E_DTYPE, "bad dtype");
    if (n_state < 1 || n_ctrl < 1 || N < 0) return fail(MPC_E_DIMS, "need n_state>=1, n_ctrl>=1, N>=0");
    if (N == 0) return MPC_OK;
    if (!x || !u || !F || !f) return fail(MPC_E_NULL, "mlp_linearize: NULL argument");
    return launch_nn64_linearize(net, (long)N, n_state, n_ctrl, (const double *)x, (const double *)u, (double *)F, (double *)f,
                                 workspace, workspace_bytes, (hipStream_t)stream);
}

int64_t mpc_mlp_param_grad_workspace_bytes(const mpc_mlp_dynamics *net, int64_t N) { return nn_param_grad_workspace_bytes(net, N); }

int mpc_mlp_param_grad(const mpc_mlp_dynamics *net, int n_state, int n_ctrl, int64_t N, const void *x, const void *u,
                       const void *gF, const void *gf, const mpc_mlp_param_grads *out, void *workspace,
                       int64_t workspace_bytes, void *stream)
{
    if (n_state < 1 || n_ctrl < 1 || N < 0) return fail(MPC_E_DIMS, "need n_state>=1, n_ctrl>=1, N>=0");
    if (!net || !out || !workspace) return fail(MPC_E_NULL, "mlp_param_grad: NULL argument");
    if (N > 0 && (!x || !u || !gF || !gf)) return fail(MPC_E_NULL, "mlp_param_grad: NULL argument");
    if (net->n_layers >= 1 && net->n_layers <= MPC_MLP_MAX_LAYERS)
        for (int l = 0; l < net->n_layers; ++l)
            if (!out->gW[l] || !out->gb[l]) return fail(MPC_E_NULL, "mlp_param_grad: gradient pointer is NULL");
    return launch_nn_param_grad(net, (long)N, n_state, n_ctrl, (const float *)x, (const float *)u, (const float *)gF,
                                (const float *)gf, out, workspace, workspace_bytes, (hipStream_t)stream);
}

// (6d') the weight gradient with a dtype: MPC_F32 is the entries above, MPC_F64 the kernels of nn_param_grad64.h
int mpc_mlp_param_grad_supported_dtype(const mpc_mlp_dynamics *net, int n_state, int n_ctrl, int dtype)
{
    if (dtype == MPC_F32) return (nn_budget(net, n_state, n_ctrl) & 4) ? 1 : 0;
    return dtype == MPC_F64 ? nn64_param_grad_supported(net, n_state, n_ctrl) : 0;
}

int64_t mpc_mlp_param_grad_workspace_bytes_dtype(const mpc_mlp_dynamics *net, int dtype, int64_t N)
{
    if (dtype == MPC_F32) return nn_param_grad_workspace_bytes(net, N);
    return dtype == MPC_F64 ? nn64_param_grad_workspace_bytes(net, N) : -1;
}

int mpc_mlp_param_grad_dtype(const mpc_mlp_dynamics *net, int dtype, int n_state, int n_ctrl, int64_t N, const void *x, const void *u,
                             const void *gF, const void *gf, const mpc_mlp_param_grads *out, void *workspace,
                             int64_t workspace_bytes, void *stream)
{
    if (dtype == MPC_F32) return mpc_mlp_param_grad(net, n_state, n_ctrl, N, x, u, gF, gf, out, workspace, workspace_bytes, stream);
    if (dtype != MPC_F64) return fail(MPC_E_DTYPE, "bad dtype");
    if (n_state < 1 || n_ctrl < 1 || N < 0) return fail(MPC_E_DIMS, "need n_state>=1, n_ctrl>=1, N>=0");
    if (!net || !out || !workspace) return fail(MPC_E_NULL, "mlp_param_grad: NULL argument");
    if (N > 0 && (!x || !u || !gF || !gf)) return fail(MPC_E_NULL, "mlp_param_grad: NULL argument");
    if (net->n_layers >= 1 && net->n_layers <= MPC_MLP_MAX_LAYERS)
        for (int l = 0; l < net->n_layers; ++l)
            if (!out->gW[l] || !out->gb[l]) return fail(MPC_E_NULL, "mlp_param_grad: gradient pointer is NULL");
    return launch_nn64_param_grad(net, (long)N, n_state, n_ctrl, (const double *)x, (const double *)u, (const double *)gF,
                                  (const double *)gf, out, workspace, workspace_bytes, (hipStream_t)stream);
}

int mpc_lqr_kkt_prepare(int dtype, int B, int T, int ns, int nc, const void *dl_dx, const void *dl_du,
                        const void *u_star, const mpc_lqr_options *o, void *negr, uint8_t *mask, void *stream)
{
    if (dtype != MPC_F32 && dtype != MPC_F64) return fail(MPC_E_DTYPE, "bad dtype");
    if (B < 0 || T < 1 || ns < 1 || nc < 1) return fail(MPC_E_DIMS, "bad dims");
    if (B == 0) return MPC_OK;
    if (!dl_dx || !dl_du || !negr) return fail(MPC_E_NULL, "kkt_prepare: NULL argument");
    const int mode = o ? o->bound_mode : MPC_BOUND_NONE;
    if (mask && (mode == MPC_BOUND_NONE || !u_star)) return fail(MPC_E_ARG, "kkt_prepare: mask needs bounds and u*");
    if (mask && mode == MPC_BOUND_TENSOR && (!o->lo || !o->hi)) return fail(MPC_E_NULL, "tensor bounds are NULL");
    return by_dtype(dtype, [&](auto t) {
        typedef decltype(t) real;
        return launch_kkt_prepare<real>(B, T, ns, nc, (const real *)dl_dx, (const real *)dl_du, (const real *)u_star, mode, o ? (real)o->lo_s : 0,
                                        o ? (real)o->hi_s : 0, o ? (const real *)o->lo : nullptr, o ? (const real *)o->hi : nullptr, (real *)negr,
                                        mask, (hipStream_t)stream);
    });
}

int mpc_pnqp_lu(int dtype, int B, int n, const void *H, const void *q, const void *lo, const void *hi,
                const void *x0, int n_iter, void *x, uint8_t *If_out, int32_t *iters, int32_t *status,
                void *Hfree, void *LU, int32_t *pivots, void *stream)
{
    if (dtype != MPC_F32 && dtype != MPC_F64) return fail(MPC_E_DTYPE, "bad dtype");
    if (B < 0 || n < 1) return fail(MPC_E_DIMS, "bad dims");
    if (B == 0) return MPC_OK;
    if (!H || !q || !lo || !hi || !x) return fail(MPC_E_NULL, "pnqp: NULL argument");
    if (n_iter < 1) n_iter = 20;
    return by_dtype(dtype, [&](auto t) {
        typedef decltype(t) real;
        return launch_pnqp<real>(B, n, (const real *)H, (const real *)q, (const real *)lo, (const real *)hi, (const real *)x0, n_iter, (real *)x,
                                 If_out, iters, status, (real *)Hfree, (real *)LU, pivots, (hipStream_t)stream);
    });
}

int mpc_pnqp(int dtype, int B, int n, const void *H, const void *q, const void *lo, const void *hi,
             const void *x0, int n_iter, void *x, uint8_t *If_out, int32_t *iters, int32_t *status,
             void *Hfree, void *stream)
{
    return mpc_pnqp_lu(dtype, B, n, H, q, lo, hi, x0, n_iter, x, If_out, iters, status, Hfree, nullptr, nullptr, stream);
}

int mpc_traj_cost(const mpc_lqr_problem *p, void *x, void *cost, void *stream)
{
    if (!p) return fail(MPC_E_NULL, "problem is NULL");
    int rc = check_problem(p, cost != nullptr, false);
    if (rc) return rc;
    if (p->B == 0) return MPC_OK;
    if (!p->cur_u) return fail(MPC_E_NULL, "traj_cost: u (cur_u) is NULL");
    hipStream_t st = (hipStream_t)stream;
    if (p->dtype == MPC_F32) {
        StepParams<float> sp = make_params<float>(p, nullptr, nullptr);
        if (!cost && x && traj_wave_supported(sp)) return launch_traj_wave(sp, (float *)x, st);
        return launch_traj_cost<float>(sp, (float *)x, (float *)cost, st);
    }
    StepParams<double> sp = make_params<double>(p, nullptr, nullptr);
    return launch_traj_cost<double>(sp, (double *)x, (double *)cost, st);
}

int mpc_select_best(int dtype, int B, int T, int ns, int nc, int first, double best_cost_eps, const void *x,
                    const void *u, const void *costs, const void *du_norm, void *best_x, void *best_u,
                    void *best_costs, void *best_du_norm, void *flags, void *host_flags, int32_t host_tag,
                    const int32_t *status, void *stream)
{
    if (dtype != MPC_F32 && dtype != MPC_F64) return fail(MPC_E_DTYPE, "bad dtype");
    if (B < 0 || T < 1 || ns < 1 || nc < 1) return fail(MPC_E_DIMS, "bad dims");
    if (B == 0) return MPC_OK;
    if (!x || !u || !costs || !du_norm || !best_x || !best_u || !best_costs || !best_du_norm || !flags)
        return fail(MPC_E_NULL, "select_best: NULL argument");
    if ((uintptr_t)flags & 7 || (uintptr_t)host_flags & 7) return fail(MPC_E_ARG, "select_best: the flags blocks must be 8-byte aligned");
    return by_dtype(dtype, [&](auto t) {
        typedef decltype(t) real;
        return launch_select_best<real>(B, T, ns, nc, first, (real)best_cost_eps, (const real *)x, (const real *)u, (const real *)costs,
                                        (const real *)du_norm, (real *)best_x, (real *)best_u, (real *)best_costs, (real *)best_du_norm, flags,
                                        host_flags, host_tag, status, (hipStream_t)stream);
    });
}

int mpc_du_norm_reference(int dtype, int T, int B, int nc, const void *u, const void *new_u, void *out, void *stream)
{
    if (dtype != MPC_F32 && dtype != MPC_F64) return fail(MPC_E_DTYPE, "bad dtype");
    if (B < 0 || T < 1 || nc < 1) return fail(MPC_E_DIMS, "bad dims");
    if (B == 0) return MPC_OK;
    if (!u || !new_u || !out) return fail(MPC_E_NULL, "du_norm_reference: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MPC_F32) return launch_du_norm_reference<float>(T, B, nc, (const float *)u, (const float *)new_u, (float *)out, st);
    return launch_du_norm_reference<double>(T, B, nc, (const double *)u, (const double *)new_u, (double *)out, st);
}

}  // extern "C"
