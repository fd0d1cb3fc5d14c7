"""CPU-only: the envelope of the network kernels (csrc/nn_dynamics.hip) as the host asks for it.  From 17 to 32 states the
output layer and the state are two 16-row accumulator tiles; the library's own budget test (mpc_mlp_supported) and the
Python gates in front of it (MlpSpec.supported, CtrlPassthroughDynamics.native_net) must offer the kernels exactly that."""
import ctypes

import torch

from mpc import _native


def test_networks_of_up_to_32_states_are_taken():
    W = _native.MlpSpec.widths_supported
    assert W([40, 100, 32])                     # BASELINE configuration 5's shape with the reference's default network
    assert W([37, 64, 48, 32])
    assert W([20, 17])                          # a single Linear layer, one state past the old limit
    assert W([25, 64, 20])
    assert not W([49, 100, 33])                 # n_state = 33: a third tile does not exist
    # what held before holds still (tests/test_host_logic.py pins more of these)
    assert W([16, 100, 12]) and W([24, 256, 32, 20, 16]) and not W([5, 1024, 4])


def test_the_lds_budget_still_refuses_a_too_wide_layer_at_32_states():
    """The second state tile lives in registers: the staging areas keep their formulas, and a layer that did not fit them
    with 16 states does not fit them with 32 (each bit of mpc_mlp_supported is one kernel's budget)."""
    W = _native.MlpSpec.widths_supported
    assert not W([40, 1024, 32]) and not W([40, 512, 512, 32])
    L = _native.load()
    e = _native.MlpDynamics()
    e.n_layers = 2
    e.widths[0], e.widths[1], e.widths[2] = 40, 1024, 32
    # rollout staging: 2 x 16 x (48 + 4) + 2 x 16 x (1024 + 4) floats = 135 KiB -- fits; the Jacobian's two product buffers do not
    assert int(L.mpc_mlp_supported(ctypes.byref(e), 32, 8)) == 1
    e.widths[1] = 100
    assert int(L.mpc_mlp_supported(ctypes.byref(e), 32, 8)) == 3
    assert int(L.mpc_mlp_supported(ctypes.byref(e), 33, 7)) == 0
    e.widths[0], e.widths[2] = 41, 33
    assert int(L.mpc_mlp_supported(ctypes.byref(e), 33, 8)) == 0


def test_the_entry_points_name_the_new_limit_without_gpu():
    """mlp_prepare: 32 states pass its shape test (the call then stops at the missing workspace), 33 do not."""
    L = _native.load()
    e = _native.MlpDynamics()
    e.n_layers, e.activation, e.passthrough = 2, 0, 1
    e.widths[0], e.widths[1], e.widths[2] = 40, 100, 32
    assert L.mpc_mlp_workspace_bytes(ctypes.byref(e)) == 4 * (112 * 52 + 112 + 32 * 116 + 32) + 256
    assert L.mpc_mlp_linearize(ctypes.byref(e), 32, 8, 8, 16, 16, 16, 16, None, 0, None) == -5
    assert b"workspace" in L.mpc_lqr_last_error()
    e.widths[0], e.widths[2] = 41, 33
    assert L.mpc_mlp_linearize(ctypes.byref(e), 33, 8, 8, 16, 16, 16, 16, 16, 1 << 20, None) == -1
    assert b"n_state <= 32" in L.mpc_lqr_last_error()


def test_python_gates_follow_the_kernels(monkeypatch):
    from mpc.dynamics import CtrlPassthroughDynamics, NNDynamics
    # MlpSpec.supported's own shape test comes before the device test: a CPU tensor is refused either way, so ask it what
    # it would say of the widths alone through a stand-in that is "on the device"
    class OnDevice:
        is_cuda, dtype = True, torch.float32

        def __init__(self, rows, cols):
            self.shape = (rows, cols)
    net = lambda widths: [OnDevice(o, i) for i, o in zip(widths, widths[1:])]
    assert _native.MlpSpec.supported(net([40, 100, 32]), "sigmoid", OnDevice(1, 1))
    assert _native.MlpSpec.supported(net([25, 64, 20]), "relu", OnDevice(1, 1))
    assert not _native.MlpSpec.supported(net([49, 100, 33]), "sigmoid", OnDevice(1, 1))
    assert not _native.MlpSpec.supported(net([40, 1024, 32]), "sigmoid", OnDevice(1, 1))
    # the slew-rate augmentation: state (previous control, x) of up to 32 entries
    monkeypatch.setattr(_native.MlpSpec, "supported", staticmethod(lambda weights, activation, like: True))
    like = torch.zeros(1)
    assert NNDynamics(32, 8, [8]).native_net(like) is not None
    aug = CtrlPassthroughDynamics(NNDynamics(28, 4, [8])).native_net(like)
    assert aug is not None and aug.n_state == 32 and aug.n_ctrl == 4 and aug.ctrl_carry == 4
    assert CtrlPassthroughDynamics(NNDynamics(29, 4, [8])).native_net(like) is None
    assert CtrlPassthroughDynamics(NNDynamics(13, 4, [8])).native_net(like) is not None      # 17: refused before
