"""What the host side of the step entry answers WITHOUT a device: mpc_lqr_impl_supported, mpc_lqr_workspace_bytes,
mpc_lqr_qp_record, mpc_lqr_kkt_fused_supported / _workspace_bytes, and the code + mpc_lqr_last_error() text with which
mpc_lqr_step, mpc_lqr_sweep, mpc_lqr_rollout and mpc_lqr_kkt_fused refuse a list of calls.

The table (step_route_answers.json) is recorded from a build of the commit BEFORE the routing of the step was gathered into one
decision (docs/history/r15.md): build that commit somewhere, then

    MPC_LQR_HIP_LIB=/path/to/that/libmpc_lqr_hip.so python tests/golden/make_golden_step_route.py

tests/test_step_route_host.py recomputes every row with `answers()` below on the library under test and compares exactly.  Only
entries that commit already has are called, through a binding of this file's own (`bind`).

No recorded call may reach a kernel launch: the pointers are made up, and the test also runs where there is a device.  So every
call of the refusal table is refused BY CONSTRUCTION -- chosen by reading the ladder, never by trying -- on a [T,B] = [5,3]
problem whose tensors are all there and 16-byte aligned, with every output, out->K / out->k and a full aligned workspace unless
the variant says otherwise.  `small` = n_state <= 12 and n_ctrl <= 4, `tiny` = n_ctrl == 1 and n_state <= 6:

  forced<i>        impl i on a shape / dtype it does not take: 2 where not small; 3 where not 12/4 or float64; 8 where not small or
                   float64; 4 where not tiny; 6 where not tiny or float64; 5 in float32 where not 32/8, in float64 where not small
                   (a small float64 problem with a workspace runs on the fused float64 kernel whatever impl says); 7 in float32 beyond
                   32/8 (in float64 impl 7 is not refused)
  nows<i>          workspace NULL: impl 0, 1, 5 (and 7 in float32) without out->K / out->k -- every path needs the workspace
                   then --, impl 2, 3, 4, 6, 8 with them (refused for the shape, or for the workspace their kernel cannot do without)
  short<i>         the same with a 16-byte workspace (every need is at least 2 T B reals)
  misaligned<i>    a full workspace 4 bytes off: impl 2, 3, 8 (and 7 in float32); under impl 0 only float32 small shapes that
                   are not tiny (the lane-per-problem kernels and the generic ones take any alignment)
  K_only           out->K without out->k: forced impl 2 (every shape: the pair is checked, or the shape refused, first); impl 0 in
                   float32 where not tiny, in float64 where small and not tiny
  sweep_nogains    MPC_OPT_SWEEP_ONLY without out->K / out->k
  sweep_entry      MPC_OPT_SWEEP_ONLY on mpc_lqr_sweep
  sweep_env        MPC_OPT_SWEEP_ONLY with a simulator (refused as such, or because the shape is not the simulator's)
  sweep_forced<i>  MPC_OPT_SWEEP_ONLY on impl 2, 4, 6: kernels that cannot stop after their sweep
  carry<i>         the cart-pole with MPC_ENV_CTRL_CARRY (6/1: refused off the lane-per-problem kernel; any other shape: not the
                   simulator's) on every forced impl -- except 4 at 6/1, which takes it --, and on mpc_lqr_sweep / mpc_lqr_rollout
  sweep_nok, rollout_nok, rollout_nox    the two-call path without gains / without new_x
  kkt_*            mpc_lqr_kkt_fused: df without f, no C_SYMMETRIC, no / short / misaligned workspace, dx_out without du_out
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "mpc.pytorch_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "step_route_answers.json")
SHAPES = ((1, 1), (3, 1), (6, 1), (7, 1), (5, 3), (12, 4), (13, 4), (12, 5), (20, 5), (32, 8), (33, 8), (32, 9), (48, 16), (63, 1))
SIZES = ((1, 1), (5, 3), (64, 1030))               # (T, B) of the workspace queries
QUERY_SIZES = ((1, 1), (200, 8))                   # ... of mpc_lqr_impl_supported (the row-per-problem kernel's LDS rule looks at T)
QP_IMPLS = (0, 3, 5, 7)
E_LAUNCH = -4
PTR, WS = 1 << 20, 1 << 24                         # made-up device addresses, 16-byte aligned: nothing recorded here dereferences one
ENV_CARTPOLE, ENV_CTRL_CARRY, OPT_SWEEP_ONLY, OPT_C_SYMMETRIC = 3, 0x100, 2, 4


def bind(native):
    """The library under MPC_LQR_HIP_LIB / beside the package, with the argument types of the entries this table calls."""
    L = ctypes.CDLL(native.lib_path())
    PP, OP, UP = ctypes.POINTER(native.Problem), ctypes.POINTER(native.Options), ctypes.POINTER(native.Outputs)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.mpc_lqr_last_error.restype = ctypes.c_char_p
    L.mpc_lqr_workspace_bytes.restype = i64
    L.mpc_lqr_workspace_bytes.argtypes = [PP]
    L.mpc_lqr_impl_supported.argtypes = [PP, OP, ctypes.c_int]
    L.mpc_lqr_qp_record.argtypes = [PP, OP, ctypes.c_int] + [ctypes.POINTER(i64)] * 3
    L.mpc_lqr_step.argtypes = [PP, OP, UP, vp, i64, ctypes.c_int, vp]
    L.mpc_lqr_sweep.argtypes = [PP, OP, UP, vp]
    L.mpc_lqr_rollout.argtypes = [PP, OP, UP, vp, vp]
    L.mpc_lqr_kkt_fused_supported.argtypes = [PP, OP]
    L.mpc_lqr_kkt_fused_workspace_bytes.restype = i64
    L.mpc_lqr_kkt_fused_workspace_bytes.argtypes = [PP]
    L.mpc_lqr_kkt_fused.argtypes = [PP, OP] + [vp] * 11 + [i64, vp]
    return L


def problem(native, ns, nc, dtype, T, B, ptr=PTR, skew=0, f=True):
    """A complete problem over made-up addresses; skew: elements added to every T / B stride."""
    p, n = native.Problem(), ns + nc
    p.B, p.T, p.ns, p.nc, p.dtype = B, T, ns, nc, dtype
    p.x_init = p.C = p.c = p.F = p.cur_x = p.cur_u = ptr
    p.C_st, p.C_sb, p.c_st, p.c_sb = B * n * n + skew, n * n + skew, B * n + skew, n + skew
    p.F_st, p.F_sb = B * ns * n + skew, ns * n + skew
    if f:
        p.f, p.f_st, p.f_sb = ptr, B * ns + skew, ns + skew
    return p


def options(native, box=0, max_ls=10, flags=0, env=None):
    """box: 0 none, 1 scalar, 2 tensor.  env: (kind, linearize) -> (Options, the struct it points to)."""
    o = native.Options()
    o.max_linesearch_iter, o.linesearch_decay, o.delta_u, o.pnqp_iter, o.flags = max_ls, 0.2, float("nan"), 20, flags
    o.bound_mode, o.lo_s, o.hi_s = box, -1.0, 1.0
    if box == 2:
        o.lo = o.hi = PTR
    e = None
    if env is not None:
        e = native.EnvDynamics()
        e.kind, e.linearize, e.params, e.dt, e.u_max = env[0], env[1], PTR, 0.05, 2.0
        o.true_dynamics = ctypes.pointer(e)
    return o, e


def outputs(native, gains=True, K_only=False, new_x=True):
    out = native.Outputs()
    for name, _ in native.Outputs._fields_:
        setattr(out, name, PTR)
    if not gains:
        out.K = out.k = None
    if K_only:
        out.k = None
    if not new_x:
        out.new_x = None
    return out


def query_options(native):
    """(name, Options or None) of the mpc_lqr_impl_supported table."""
    rows = [("none", None), ("default", options(native)), ("box", options(native, box=1)), ("ls16", options(native, max_ls=16)),
            ("ls17", options(native, max_ls=17))]
    for kind, carry, lin in itertools.product((1, 2, 3), (0, 1), (0, 1)):
        rows.append(("env%d%s%s" % (kind, "+carry" if carry else "", "+lin" if lin else ""),
                     options(native, env=(kind | (ENV_CTRL_CARRY if carry else 0), lin))))
    return rows


def step_calls(native, L, ns, nc, dtype):
    """[(variant, (p, o, out, workspace, bytes, impl))]: the mpc_lqr_step calls of the refusal table, see the module docstring
    (the structs keep what they point to alive through `_keep` attributes)."""
    f32 = dtype == native.MPC_F32
    small, tiny = ns <= 12 and nc <= 4, nc == 1 and ns <= 6
    p = problem(native, ns, nc, dtype, 5, 3)
    full = int(L.mpc_lqr_workspace_bytes(ctypes.byref(p)))
    plain, _ = options(native)
    sweep, _ = options(native, flags=OPT_SWEEP_ONLY)
    sweep_env, sweep_env._keep = options(native, flags=OPT_SWEEP_ONLY, env=(1, 0))
    carry, carry._keep = options(native, env=(ENV_CARTPOLE | ENV_CTRL_CARRY, 0))
    calls = []

    def add(name, impl, o=plain, gains=True, K_only=False, ws=WS, nbytes=full):
        calls.append((name, (p, o, outputs(native, gains=gains, K_only=K_only), ws, nbytes, impl)))

    forced = {2: not small, 3: not f32 or (ns, nc) != (12, 4), 8: not f32 or not small, 4: not tiny, 6: not f32 or not tiny,
              5: (ns, nc) != (32, 8) if f32 else not small, 7: f32 and (ns > 32 or nc > 8)}
    for i in sorted(forced):
        if forced[i]:
            add("forced%d" % i, i)
    for tag, kw in (("nows", dict(ws=None, nbytes=0)), ("short", dict(ws=WS, nbytes=16))):
        for i in (0, 1, 5) + ((7,) if f32 else ()):
            add("%s%d" % (tag, i), i, gains=False, **kw)
        for i in (2, 3, 4, 6, 8):
            add("%s%d" % (tag, i), i, **kw)
    for i in (2, 3, 8) + ((7,) if f32 else ()):
        add("misaligned%d" % i, i, ws=WS + 4)
    if f32 and small and not tiny:
        add("misaligned0", 0, gains=False, ws=WS + 4)
    add("K_only2", 2, K_only=True)
    if not tiny and (f32 or small):
        add("K_only0", 0, K_only=True)
    add("sweep_nogains", 0, o=sweep, gains=False)
    add("sweep_env", 0, o=sweep_env)
    for i in (2, 4, 6):
        add("sweep_forced%d" % i, i, o=sweep)
    for i in (1, 2, 3, 4, 5, 6, 7, 8):
        if not (i == 4 and (ns, nc) == (6, 1)):
            add("carry%d" % i, i, o=carry)
    return calls


def refusals(native, L, ns, nc, dtype):
    """{variant: [code, text]}: see the module docstring.  Every call here is refused before any launch by construction."""
    r = ctypes.byref
    got = {}

    def record(name, fn, *args):
        rc = int(fn(*args))
        got[name] = [rc, L.mpc_lqr_last_error().decode()]

    for name, (p, o, out, ws, nbytes, impl) in step_calls(native, L, ns, nc, dtype):
        record(name, L.mpc_lqr_step, r(p), r(o), r(out), ws, nbytes, impl, None)
    p = problem(native, ns, nc, dtype, 5, 3)
    plain, _ = options(native)
    sweep, _ = options(native, flags=OPT_SWEEP_ONLY)
    carry, keep_carry = options(native, env=(ENV_CARTPOLE | ENV_CTRL_CARRY, 0))
    record("sweep_entry", L.mpc_lqr_sweep, r(p), r(sweep), r(outputs(native)), None)
    record("sweep_nok", L.mpc_lqr_sweep, r(p), r(plain), r(outputs(native, gains=False)), None)
    record("sweep_carry", L.mpc_lqr_sweep, r(p), r(carry), r(outputs(native)), None)
    record("rollout_nok", L.mpc_lqr_rollout, r(p), r(plain), r(outputs(native, gains=False)), None, None)
    record("rollout_nox", L.mpc_lqr_rollout, r(p), r(plain), r(outputs(native, new_x=False)), None, None)
    record("rollout_carry", L.mpc_lqr_rollout, r(p), r(carry), r(outputs(native)), None, None)
    # mpc_lqr_kkt_fused(p, o, dl_dx, dl_du, dC, dc, dF, df, dx_init, dx_out, du_out, status, workspace, bytes, stream)
    sym, _ = options(native, flags=OPT_C_SYMMETRIC)
    kfull = int(L.mpc_lqr_kkt_fused_workspace_bytes(r(p)))
    nof = problem(native, ns, nc, dtype, 5, 3, f=False)
    grads = (PTR,) * 9                        # dl_dx, dl_du, dC, dc, dF, df, dx_init, dx_out, du_out
    record("kkt_df_without_f", L.mpc_lqr_kkt_fused, r(nof), r(sym), *grads, None, WS, kfull, None)
    record("kkt_not_symmetric", L.mpc_lqr_kkt_fused, r(p), r(plain), *grads, None, WS, kfull, None)
    record("kkt_nows", L.mpc_lqr_kkt_fused, r(p), r(sym), *grads, None, None, 0, None)
    record("kkt_short", L.mpc_lqr_kkt_fused, r(p), r(sym), *grads, None, WS, 16, None)
    record("kkt_misaligned", L.mpc_lqr_kkt_fused, r(p), r(sym), *grads, None, WS + 4, kfull, None)
    record("kkt_dx_without_du", L.mpc_lqr_kkt_fused, r(p), r(sym), *grads[:8], None, None, WS, kfull, None)
    del keep_carry
    for name, (rc, text) in got.items():
        assert rc not in (0, E_LAUNCH), "%s (%d/%d, dtype %d) was meant to be refused before any launch: %d %s" % (name, ns, nc, dtype, rc, text)
    return got


def answers(native, L, ns, nc, dtype):
    """One row of the table, from the library `L` (mpc._native as `native` for the structs)."""
    r = ctypes.byref
    row = {"n_state": ns, "n_ctrl": nc, "dtype": dtype}
    # mpc_lqr_impl_supported: {options: [[impl 0..8] for each of QUERY_SIZES]}
    row["impl_supported"] = {}
    for name, ok in query_options(native):
        o = None if ok is None else r(ok[0])
        row["impl_supported"][name] = ["".join(str(int(L.mpc_lqr_impl_supported(r(problem(native, ns, nc, dtype, T, B)), o, impl)))
                                               for impl in range(9)) for T, B in QUERY_SIZES]
    row["workspace_bytes"] = [int(L.mpc_lqr_workspace_bytes(r(problem(native, ns, nc, dtype, T, B)))) for T, B in SIZES]
    # mpc_lqr_qp_record at [5,3]: {alignment: {bounds: [[filled, offset, st, sb] for impl in QP_IMPLS]}}
    row["qp_record"] = {}
    for align, kw in (("aligned", {}), ("pointers+4", dict(ptr=PTR + 4)), ("strides+1", dict(skew=1))):
        p = problem(native, ns, nc, dtype, 5, 3, **kw)
        row["qp_record"][align] = {}
        for box in (0, 1, 2):
            o, _ = options(native, box=box)
            cell = []
            for impl in QP_IMPLS:
                off, st, sb = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_int64(-7)
                ok = int(L.mpc_lqr_qp_record(r(p), r(o), impl, r(off), r(st), r(sb)))
                cell.append([ok, off.value, st.value, sb.value])
            row["qp_record"][align]["box%d" % box] = cell
    # the fused KKT backward's queries
    kkt = {}
    for name, o in (("none", None), ("default", options(native)), ("symmetric", options(native, flags=OPT_C_SYMMETRIC)),
                    ("symmetric+box", options(native, box=1, flags=OPT_C_SYMMETRIC)),
                    ("symmetric+env", options(native, flags=OPT_C_SYMMETRIC, env=(1, 0)))):
        kkt[name] = int(L.mpc_lqr_kkt_fused_supported(r(problem(native, ns, nc, dtype, 5, 3)), None if o is None else r(o[0])))
    row["kkt_fused_supported"] = kkt
    row["kkt_fused_workspace_bytes"] = [int(L.mpc_lqr_kkt_fused_workspace_bytes(r(problem(native, ns, nc, dtype, T, B)))) for T, B in SIZES]
    row["refusals"] = refusals(native, L, ns, nc, dtype)
    return row


def rows(native, L):
    return [answers(native, L, ns, nc, dtype) for ns, nc in SHAPES for dtype in (native.MPC_F32, native.MPC_F64)]


def pack(table):
    """The texts once, the rows referring to them by index."""
    texts = sorted({t for row in table for _, t in row["refusals"].values()})
    for row in table:
        row["refusals"] = {k: [rc, texts.index(t)] for k, (rc, t) in row["refusals"].items()}
    return {"texts": texts, "rows": table}


def unpack(table):
    for row in table["rows"]:
        row["refusals"] = {k: [rc, table["texts"][i]] for k, (rc, i) in row["refusals"].items()}
    return table["rows"]


def main():
    from mpc import _native
    table = pack(rows(_native, bind(_native)))
    with open(OUT, "w") as fh:
        fh.write('{"texts": %s,\n "rows": [\n' % json.dumps(table["texts"]))
        fh.write(",\n".join("  " + json.dumps(row, separators=(",", ":")) for row in table["rows"]))
        fh.write("\n ]}\n")
    print("%s: %d rows, %d bytes, library %s" % (OUT, len(table["rows"]), os.path.getsize(OUT), _native.lib_path()))


if __name__ == "__main__":
    main()
