"""Host-side checks of the 5x5 convolution route (ebfi_conv5x5_* of include/ebfi_hip.h, ebfi_amd.conv): the entry points are
declared, bound and exported; every refusal happens before the GPU is touched; `conv.supported` on CPU-made metadata; and the
float64 restatement of the recurrent U-Nets (tests/unet_ref.py) at kernel_size=5 against the reference's own numbers
(tests/golden/unet_k5_small.npz, written by tests/golden/make_unet_k5_golden.py).  Nothing here computes on a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ref as R  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd import conv  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "unet_k5_small.npz")
ENTRY_POINTS = ("ebfi_conv5x5_forward", "ebfi_conv5x5_backward_data", "ebfi_conv5x5_backward_weight")
WORKSPACE = "ebfi_conv5x5_backward_weight_workspace"
ERR_ARG, ERR_UNSUPPORTED = N.CONSTANTS["EBFI_ERR_ARG"], N.CONSTANTS["EBFI_ERR_UNSUPPORTED"]
ERR_WORKSPACE = N.CONSTANTS["EBFI_ERR_WORKSPACE"]


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


@pytest.fixture()
def k5():
    """tests/unet_ref.py restated at kernel_size=5; the module's configuration is put back afterwards."""
    before = R.CFG["kernel_size"]
    R.CFG["kernel_size"] = 5
    try:
        yield R
    finally:
        R.CFG["kernel_size"] = before


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_bound_and_exported_at_abi_14(built_lib):
    assert N.ABI_VERSION == 14 == built_lib.ebfi_abi_version()
    declared = N.declared_symbols()
    h = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRY_POINTS + (WORKSPACE,):
        assert name in declared and name in N.SIGNATURES and hasattr(h, name) and hasattr(built_lib, name), name
    for name in ENTRY_POINTS:
        assert N.PARAMS[name][-1] == "void *stream" and N.SIGNATURES[name][0] is ctypes.c_int
    assert N.SIGNATURES[WORKSPACE] == (ctypes.c_size_t, [ctypes.c_int] * 7)
    assert len(N.PARAMS["ebfi_conv5x5_forward"]) == 14 and len(N.PARAMS["ebfi_conv5x5_backward_data"]) == 14
    assert len(N.PARAMS["ebfi_conv5x5_backward_weight"]) == 18
    assert [p.split()[-1].lstrip("*") for p in N.PARAMS["ebfi_conv5x5_backward_weight"][:6]] == \
        ["input", "grad_output", "saved_output", "grad_weight", "grad_bias", "grad_preact_out"]


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu(built_lib):
    """(No GPU here: a launch, a memset or a stream query would fail or crash instead of returning these codes.)"""
    lib = built_lib
    p = ctypes.c_void_p(4096)
    err = lambda: lib.ebfi_last_error()
    geo = (1, 3, 8, 8, 4, 2, 2)                                # B, Cin, H, W, Cout, stride, pad
    fwd = lambda *a, g=geo, act=0: lib.ebfi_conv5x5_forward(*a, *g, act, 0.0, None)
    dgr = lambda *a, g=geo, act=0: lib.ebfi_conv5x5_backward_data(*a, *g, act, 0.0, None)
    wgr = lambda *a, g=geo, act=0, ws=p, nbytes=1 << 40: lib.ebfi_conv5x5_backward_weight(*a, *g, act, 0.0, ws, nbytes, None)
    # null pointers (bias, saved_output without activation, grad_bias and grad_preact_out may be NULL: not refused for that)
    assert fwd(None, p, p, p) == ERR_ARG and b"null" in err()
    assert fwd(p, None, p, p) == ERR_ARG and b"null" in err()
    assert fwd(p, p, None, None) == ERR_ARG and b"null" in err()
    assert dgr(None, None, p, p) == ERR_ARG and b"null" in err()
    assert dgr(p, None, None, p) == ERR_ARG and b"null" in err()
    assert dgr(p, None, p, None) == ERR_ARG and b"null" in err()
    assert wgr(None, p, None, p, None, None) == ERR_ARG and b"null" in err()
    assert wgr(p, None, None, p, None, None) == ERR_ARG and b"null" in err()
    assert wgr(p, p, None, None, None, None) == ERR_ARG and b"null" in err()
    # an activation without saved_output; an unknown activation
    for act in (1, 2):
        assert dgr(p, None, p, p, act=act) == ERR_ARG and b"saved_output" in err()
        assert wgr(p, p, None, p, p, p, act=act) == ERR_ARG and b"saved_output" in err()
    assert fwd(p, p, p, p, act=3) == ERR_ARG and dgr(p, p, p, p, act=-1) == ERR_ARG and wgr(p, p, p, p, p, p, act=7) == ERR_ARG
    # stride 3 (and 0), pad 5 (and -1)
    for bad, word in (((1, 3, 8, 8, 4, 3, 2), b"stride"), ((1, 3, 8, 8, 4, 0, 2), b"stride"), ((1, 3, 8, 8, 4, 1, 5), b"padding"),
                      ((1, 3, 8, 8, 4, 2, 5), b"padding"), ((1, 3, 8, 8, 4, 2, -1), b"padding")):
        assert fwd(p, p, p, p, g=bad) == ERR_UNSUPPORTED and word in err()
        assert dgr(p, None, p, p, g=bad) == ERR_UNSUPPORTED and word in err()
        assert wgr(p, p, None, p, p, None, g=bad) == ERR_UNSUPPORTED and word in err()
        assert lib.ebfi_conv5x5_backward_weight_workspace(*bad) == 0
    # an empty output; non-positive sizes
    for bad, word in (((1, 3, 4, 8, 4, 1, 0), b"empty"), ((1, 3, 8, 2, 4, 2, 1), b"empty"), ((1, 0, 8, 8, 4, 1, 2), b"dimension"),
                      ((1, 3, 8, 8, 0, 1, 2), b"dimension"), ((-1, 3, 8, 8, 4, 1, 2), b"dimension"), ((1, 3, 0, 8, 4, 1, 2), b"dimension")):
        assert fwd(p, p, p, p, g=bad) == ERR_ARG and word in err()
        assert dgr(p, None, p, p, g=bad) == ERR_ARG and word in err()
        assert wgr(p, p, None, p, p, None, g=bad) == ERR_ARG and word in err()
        assert lib.ebfi_conv5x5_backward_weight_workspace(*bad) == 0
    # a sample beyond the 2 GiB reach of the 32-bit buffer offsets
    assert fwd(p, p, p, p, g=(1, 64, 4096, 4096, 4, 1, 2)) == ERR_ARG and b"2 GiB" in err()
    # a missing or short workspace
    need = lib.ebfi_conv5x5_backward_weight_workspace(*geo)
    assert need >= (4 * 3 * 25 + 4) * 4 and need % ((4 * 3 * 25 + 4) * 4) == 0
    assert wgr(p, p, None, p, p, None, ws=None) == ERR_WORKSPACE and b"workspace" in err()
    assert wgr(p, p, None, p, p, None, nbytes=need - 1) == ERR_WORKSPACE and b"workspace" in err()
    assert wgr(p, p, None, p, p, None, nbytes=0) == ERR_WORKSPACE
    # the workspace of the flagship shapes: one slab per workgroup of one resident round (at most 512)
    for g in ((8, 32, 256, 256, 64, 2, 2), (8, 64, 256, 256, 32, 1, 2), (8, 5, 256, 256, 32, 1, 2)):
        slab = (g[4] * g[1] * 25 + g[4]) * 4
        n = lib.ebfi_conv5x5_backward_weight_workspace(*g)
        assert n % slab == 0 and 1 <= n // slab <= 512


def test_the_older_entry_points_refuse_what_they_refused(built_lib):
    """ebfi_conv2d_* keep their limits (argument checks only: they return before any launch)."""
    lib = built_lib
    p = ctypes.c_void_p(4096)
    geo = (1, 8, 8, 8, 8, 5)
    assert lib.ebfi_conv2d_forward(p, p, None, p, *geo, 2, 2, 0, 0.0, N.EBFI_F32, None) == ERR_UNSUPPORTED
    assert lib.ebfi_conv2d_backward_data(p, None, p, p, *geo, 1, 2, 0, 0.0, N.EBFI_F32, None) == ERR_UNSUPPORTED
    assert lib.ebfi_conv2d_backward_weight_workspace(*geo, 1, 2, N.EBFI_F32) == 0
    assert lib.ebfi_conv2d_backward_weight_workspace(*geo, 2, 2, N.EBFI_F32) == 0
    # and the sizes they hand out for their own kernel sizes are what the slab scheme of each gives
    for k, s, cib in ((3, 1, 64), (3, 2, 32), (7, 1, 8), (7, 2, 8), (1, 1, 64)):
        n = lib.ebfi_conv2d_backward_weight_workspace(2, 16, 40, 40, 16, k, s, k // 2, N.EBFI_F32)
        slab = (16 * 16 * k * k + 16) * 4
        assert n % slab == 0 and n // slab >= 1, (k, s)


# ------------------------------------------------------------------------------------------------------------ routing
class _Meta:
    """What `conv.supported` reads of a tensor, made on the CPU: a CUDA float32 tensor's metadata."""

    def __init__(self, shape, dtype=torch.float32, is_cuda=True):
        self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, is_cuda

    def dim(self):
        return len(self.shape)


def test_supported_admits_5x5_at_stride_1_and_2_with_pad_0_to_4():
    x = _Meta((2, 4, 16, 16))
    w5 = _Meta((4, 4, 5, 5))
    for stride in (1, 2):
        for pad in range(5):
            assert conv.supported(x, w5, (stride, stride), (pad, pad)), (stride, pad)
        assert not conv.supported(x, w5, (stride, stride), (5, 5))               # stays on torch, through left_native
        assert not conv.supported(x, w5, (stride, stride), (-1, -1))
    assert not conv.supported(x, w5, (3, 3), (2, 2)) and not conv.supported(x, w5, (1, 2), (2, 2))
    assert not conv.supported(x, w5, (1, 1), (2, 1)) and not conv.supported(x, w5, (1, 1), (2, 2), (2, 2))
    assert not conv.supported(x, w5, (1, 1), (2, 2), (1, 1), 2)
    assert not conv.supported(x, _Meta((4, 4, 5, 3)), (1, 1), (2, 2))
    assert not conv.supported(_Meta((2, 4, 16, 16), is_cuda=False), w5, (1, 1), (2, 2))
    assert not conv.supported(_Meta((2, 4, 16, 16), torch.float16), w5, (1, 1), (2, 2))
    # the other kernel sizes are where they were: pad up to k, no strided 1x1, nothing else
    for k, ok in ((1, True), (3, True), (7, True), (2, False), (4, False), (6, False), (9, False)):
        wk = _Meta((4, 4, k, k))
        assert conv.supported(x, wk, (1, 1), (k // 2, k // 2)) == ok, k
        if ok:
            assert conv.supported(x, wk, (1, 1), (k, k)) and not conv.supported(x, wk, (1, 1), (k + 1, k + 1))
    assert not conv.supported(x, _Meta((4, 4, 1, 1)), (2, 2), (0, 0)) and conv.supported(x, _Meta((4, 4, 3, 3)), (2, 2), (1, 1))
    # split / single-rounding operand modes never claim a 5x5 layer: it runs exact fp32 in every mode
    for mode in conv.MODES:
        assert not conv._bf16_ok(5, 1, mode) and not conv._x3_ok(5, 1, 4, mode) and not conv._bf16_ok(5, 2, mode)


def test_left_native_is_silent_on_cpu_and_raises_for_pad_5_under_the_strict_switch(monkeypatch):
    w5 = _Meta((4, 4, 5, 5))
    monkeypatch.setenv("EBFI_STRICT_NATIVE", "1")
    conv.left_native(_Meta((1, 4, 8, 8), is_cuda=False), w5, (2, 2), (5, 5))
    with pytest.raises(N.EbfiNativeError, match="EBFI_STRICT_NATIVE"):
        conv.left_native(_Meta((1, 4, 8, 8)), w5, (2, 2), (5, 5))


# ------------------------------------------------------------------------------------------------------------ the k=5 restatement
@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / float(np.abs(want).max())


def test_the_patch_is_undone(k5):
    assert k5.CFG["kernel_size"] == 5 and dict(k5.names_and_shapes("A"))["head.conv2d.weight"] == (8, 5, 5, 5)
    assert dict(k5.names_and_shapes("A"))["encoders.0.recurrent_block.Gates.weight"][-1] == 3      # the cells stay 3x3


def test_the_configuration_is_back_at_3():
    assert R.CFG["kernel_size"] == 3


@pytest.mark.parametrize("case", list(R.CASES))
def test_k5_restatement_agrees_with_the_reference_in_float64(fixture, k5, case):
    """tests/golden/unet_k5_small.npz was written by the reference's own models/model_misc/unet.py at kernel_size=5: 1e-12 of each
    output's scale.  The stored seed keeps every ReLU pre-activation >= 1e-5 away from zero, and float32 flips no mask."""
    i = list(k5.CASES).index(case)
    seed = int(fixture["seeds"][i])
    assert 1 <= seed <= 64
    xs, cots = k5.make_inputs(seed + 1000, case)
    state = k5.fill_state(seed, case)
    got = k5.run(case, state, xs, cots)
    expect = k5.names_and_shapes(case)
    assert [str(n) for n in fixture[case + "_names"]] == [n for n, _ in expect]
    assert [str(s) for s in fixture[case + "_shapes"]] == [str(tuple(s)) for _, s in expect]
    assert fixture[case + "_out"].shape[1:] == k5.out_shape(case)
    for c in range(2):
        assert _err(got["outs"][c].numpy(), fixture[case + "_out"][c]) <= 1e-12
    states = np.concatenate([s.numpy().reshape(-1) for s in got["states"]])
    assert states.shape == fixture[case + "_states"].shape and _err(states, fixture[case + "_states"]) <= 1e-12
    table = k5.grad_table([got["grads"][n] for n, _ in expect])
    want = fixture[case + "_grads"]
    assert table.shape == want.shape
    assert _err(table[:, 0], want[:, 0]) <= 1e-12 and _err(table[:, 1:], want[:, 1:]) <= 1e-12
    # the margin of the stored seed, and the masks of a float32 run
    margin = min(float(p.abs().min()) for p in got["preacts"])
    print("k5 case %s: seed %d, smallest |ReLU pre-activation| %.3e" % (case, seed, margin))
    assert margin >= 1e-5
    got32 = k5.run(case, state, xs, cots, dtype=torch.float32)
    assert len(got32["preacts"]) == len(got["preacts"])
    flips = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(got["preacts"], got32["preacts"]))
    assert flips == 0
    assert os.path.getsize(FIXTURE) < 300 * 1024
