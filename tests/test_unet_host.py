"""Host-side checks of the recurrent U-Nets (ebfi_amd.unet, ebfi_amd.recurrent, tests/unet_ref.py): the float64 restatement
against the reference's own numbers, the import paths, the state-dict keys, the CPU fallback of the modules, the declared entry
points and every refusal.  Nothing here computes on a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_ref as R  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "unet_small.npz")
ENTRY_POINTS = ("ebfi_lstm_cell_forward", "ebfi_lstm_cell_backward", "ebfi_gru_reset_forward", "ebfi_gru_reset_backward",
                "ebfi_gru_update_forward", "ebfi_gru_update_backward", "ebfi_bilinear_up_forward", "ebfi_bilinear_up_backward")


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def restated(fixture):
    """case -> the restatement's float64 run on the fixture's seed: computed once, shared, never modified."""
    out = {}
    for i, case in enumerate(R.CASES):
        seed = int(fixture["seeds"][i])
        xs, cots = R.make_inputs(seed + 1000, case)
        out[case] = (seed, xs, cots, R.run(case, R.fill_state(seed, case), xs, cots))
    return out


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / float(np.abs(want).max())


def _build(case):
    from models.model_misc import unet
    return getattr(unet, R.CASES[case]["net"])(R.unet_kwargs(case))


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_agrees_with_the_reference_in_float64(fixture, restated, case):
    """tests/golden/unet_small.npz was written by the reference's own models/model_misc/unet.py
    (tests/golden/make_unet_golden.py).  The restatement is a different program for the same law: 1e-12 of each output's scale."""
    _, _, _, got = restated[case]
    assert fixture[case + "_out"].shape[1:] == R.out_shape(case)
    for c in range(2):
        assert _err(got["outs"][c].numpy(), fixture[case + "_out"][c]) <= 1e-12
    states = np.concatenate([s.numpy().reshape(-1) for s in got["states"]])
    assert states.shape == fixture[case + "_states"].shape and _err(states, fixture[case + "_states"]) <= 1e-12
    table = R.grad_table([got["grads"][n] for n, _ in R.names_and_shapes(case)])
    want = fixture[case + "_grads"]
    assert table.shape == want.shape
    assert _err(table[:, 0], want[:, 0]) <= 1e-12 and _err(table[:, 1:], want[:, 1:]) <= 1e-12      # the sums; the heads
    assert os.path.getsize(FIXTURE) < 300 * 1024


def test_reference_import_paths_resolve_to_the_device_classes():
    from ebfi_amd import model, recurrent, unet
    from models.model_misc.model_util import skip_concat, skip_sum
    from models.model_misc.submodules import (ConvGRU, ConvLayer, ConvLSTM, RecurrentConvLayer, ResidualBlock,
                                              TransposedConvLayer, UpsampleConvLayer)
    from models.model_misc.unet import BaseUNet, BaseUNet_legacy, SRUNetRecurrent, UNetFlow, UNetRecurrent
    assert (UNetFlow, UNetRecurrent, SRUNetRecurrent) == (unet.UNetFlow, unet.UNetRecurrent, unet.SRUNetRecurrent)
    assert (BaseUNet, BaseUNet_legacy) == (unet.BaseUNet, unet.BaseUNet_legacy)
    assert (ConvLSTM, ConvGRU, RecurrentConvLayer) == (recurrent.ConvLSTM, recurrent.ConvGRU, recurrent.RecurrentConvLayer)
    assert (ResidualBlock, UpsampleConvLayer, TransposedConvLayer) == (recurrent.ResidualBlock, recurrent.UpsampleConvLayer,
                                                                       recurrent.TransposedConvLayer)
    assert ConvLayer is model.ConvLayer and (skip_sum, skip_concat) == (unet.skip_sum, unet.skip_concat)
    # the ZeroPad2d law of the skips: a negative pad crops (an odd size up-sampled is one pixel too large)
    a, b = torch.arange(2 * 10 * 6, dtype=torch.float32).view(1, 2, 10, 6), torch.ones(1, 2, 9, 7)
    want = torch.nn.ZeroPad2d((0, 1, -1, 0))(a)
    assert torch.equal(skip_sum(a, b), want + b) and torch.equal(skip_concat(a, b), torch.cat([want, b], 1))


@pytest.mark.parametrize("case", list(R.CASES))
def test_state_dict_keys_and_shapes_are_the_references(fixture, case):
    net = _build(case)
    sd = net.state_dict()
    assert list(sd) == [str(n) for n in fixture[case + "_names"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in fixture[case + "_shapes"]]
    assert net.states == [None] * 2 and [(n, tuple(s)) for n, s in R.names_and_shapes(case)] == [(k, tuple(v.shape)) for k, v in sd.items()]
    if R.CASES[case]["recurrent_block_type"] == "convgru":             # the reference's initialisation of the GRU gates
        for gate in ("reset_gate", "update_gate", "out_gate"):
            w = sd["encoders.0.recurrent_block.%s.weight" % gate].flatten(1)
            assert torch.allclose(w @ w.t(), torch.eye(w.shape[0]), atol=1e-5)
            assert not sd["encoders.0.recurrent_block.%s.bias" % gate].any()


@pytest.mark.parametrize("case", list(R.CASES))
def test_modules_on_cpu_tensors_give_the_restatement(restated, case):
    """The fallback path (CPU tensors, float64): the modules' own expressions against the restatement, outputs, final states and
    every parameter gradient, to 1e-12 of each tensor's scale."""
    seed, xs, cots, want = restated[case]
    net = _build(case).double()
    net.load_state_dict(R.fill_state(seed, case))
    outs = [R.module_outputs(net(x)) for x in xs]
    loss = sum((c * o).sum() for c, o in zip(cots, outs))
    params = dict(net.named_parameters())
    names = [n for n, _ in R.names_and_shapes(case)]
    grads = torch.autograd.grad(loss, [params[n] for n in names])
    for got, ref in zip(outs, want["outs"]):
        assert got.shape == ref.shape and _err(got.detach().numpy(), ref.numpy()) <= 1e-12
    states = R.flat_states(net.states)
    assert len(states) == len(want["states"])
    for got, ref in zip(states, want["states"]):
        assert _err(got.detach().numpy(), ref.numpy()) <= 1e-12
    for n, g in zip(names, grads):
        assert _err(g.numpy(), want["grads"][n].numpy()) <= 1e-12, n
    if R.CASES[case]["net"] == "UNetFlow":
        out = net(xs[0])
        assert set(out) == {"image", "flow"} and out["image"].shape[1] == 1 and out["flow"].shape[1] == 2


def test_entry_points_are_declared_and_exported_at_abi_14(built_lib):
    assert N.ABI_VERSION == 14 == built_lib.ebfi_abi_version()
    declared = N.declared_symbols()
    h = ctypes.CDLL(N.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared and name in N.SIGNATURES and hasattr(h, name), name
        assert N.PARAMS[name][-1] == "void *stream" and N.SIGNATURES[name][0] is ctypes.c_int
    source = open(os.path.join(N.PKG_ROOT, "csrc", "recurrent.hip")).read()
    assert "atomic" not in source.split("#include", 1)[1].lower()         # (the file's heading says so; the code must not use one)
    assert "hipMalloc" not in source and "Synchronize" not in source


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu(built_lib):
    lib = built_lib
    p = ctypes.c_void_p(4096)
    err = lambda: lib.ebfi_last_error()
    # null required pointers
    assert lib.ebfi_lstm_cell_forward(None, p, p, p, 1, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_lstm_cell_forward(p, None, None, p, 1, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_lstm_cell_backward(p, p, None, p, p, p, p, 1, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_lstm_cell_backward(p, p, p, p, p, None, p, 1, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_gru_reset_forward(p, None, p, p, 1, 4, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_gru_reset_backward(None, p, p, None, p, p, p, 1, 4, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_gru_reset_backward(p, p, p, None, p, None, p, 1, 4, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_gru_update_forward(p, p, p, None, 1, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_gru_update_backward(p, p, p, None, p, p, p, 1, 4, 16, None) == -1 and b"null" in err()
    assert lib.ebfi_bilinear_up_forward(None, p, 1, 4, 4, 2, None) == -1 and b"null" in err()
    assert lib.ebfi_bilinear_up_backward(p, None, 1, 4, 4, 2, None) == -1 and b"null" in err()
    # non-positive sizes
    for B, C, HW in ((1, 0, 16), (1, -3, 16), (0, 4, 16), (1, 4, 0)):
        assert lib.ebfi_lstm_cell_forward(p, p, p, p, B, C, HW, None) == -1 and b"positive" in err()
        assert lib.ebfi_lstm_cell_backward(p, p, p, p, p, p, p, B, C, HW, None) == -1 and b"positive" in err()
        assert lib.ebfi_gru_update_forward(p, p, p, p, B, C, HW, None) == -1 and b"positive" in err()
        assert lib.ebfi_gru_update_backward(p, p, p, p, p, p, p, B, C, HW, None) == -1 and b"positive" in err()
        assert lib.ebfi_gru_reset_forward(p, p, p, p, B, 4, C, HW, None) == -1 and b"positive" in err()
        assert lib.ebfi_gru_reset_backward(p, p, p, p, p, p, p, B, 4, C, HW, None) == -1 and b"positive" in err()
    assert lib.ebfi_gru_reset_forward(p, p, p, p, 1, 0, 4, 16, None) == -1 and b"Cx" in err()
    assert lib.ebfi_gru_reset_backward(p, p, p, p, p, p, p, 1, 0, 4, 16, None) == -1 and b"Cx" in err()
    for planes, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert lib.ebfi_bilinear_up_forward(p, p, planes, H, W, 2, None) == -1 and b"positive" in err()
        assert lib.ebfi_bilinear_up_backward(p, p, planes, H, W, 4, None) == -1 and b"positive" in err()
    # an unsupported scale
    for scale in (3, 1, 0, 8):
        assert lib.ebfi_bilinear_up_forward(p, p, 1, 4, 4, scale, None) == -1 and b"scale" in err()
        assert lib.ebfi_bilinear_up_backward(p, p, 1, 4, 4, scale, None) == -1 and b"scale" in err()


def test_layers_keep_the_references_interfaces():
    from ebfi_amd import recurrent as M
    lstm, gru = M.ConvLSTM(4, 6, 3), M.ConvGRU(4, 6, 3)
    assert list(lstm.state_dict()) == ["Gates.weight", "Gates.bias"] and lstm.Gates.weight.shape == (24, 10, 3, 3)
    assert [k.split(".")[0] for k in gru.state_dict()][::2] == ["reset_gate", "update_gate", "out_gate"]
    x = torch.randn(2, 4, 5, 7)
    h, c = lstm(x)                                                       # prev_state=None is the default, as in the reference
    assert h.shape == c.shape == (2, 6, 5, 7) and isinstance(gru(x, None), torch.Tensor)
    h2, c2 = lstm(x, (h, c))
    assert h2.shape == (2, 6, 5, 7) and not torch.equal(h2, h)
    layer = M.RecurrentConvLayer(3, 4, kernel_size=3, stride=2, padding=1, recurrent_block_type="convgru")
    y, state = layer(torch.randn(1, 3, 8, 8), None)
    assert y is state and y.shape == (1, 4, 4, 4)
    up = M.UpsampleConvLayer(3, 5, kernel_size=3, padding=1, scale=4)
    assert list(up.state_dict()) == ["conv2d.weight", "conv2d.bias"] and up(torch.randn(1, 3, 3, 5)).shape == (1, 5, 12, 20)
    assert list(M.UpsampleConvLayer(3, 5, 3, padding=1, norm="BN").state_dict())[:3] == ["conv2d.weight", "norm_layer.weight", "norm_layer.bias"]
    tr = M.TransposedConvLayer(3, 5, kernel_size=3, padding=1)
    assert list(tr.state_dict()) == ["transposed_conv2d.weight", "transposed_conv2d.bias"] and tr(torch.randn(1, 3, 4, 4)).shape == (1, 5, 8, 8)
    rb = M.ResidualBlock(4, 4, norm="BN")
    assert list(rb.state_dict())[:2] == ["conv1.weight", "bn1.weight"] and "conv2.weight" in rb.state_dict() and rb.conv1.bias is None
    assert float(M.ResidualBlock(4, 4)(torch.randn(1, 4, 5, 5)).detach().min()) >= 0 and rb(torch.randn(2, 4, 5, 5)).shape == (2, 4, 5, 5)
    assert float(M.ResidualBlock(4, 4, final_activation=False)(torch.randn(4, 4, 5, 5)).detach().min()) < 0
