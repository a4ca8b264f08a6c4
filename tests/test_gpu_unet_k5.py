"""The recurrent U-Nets on the device at kernel_size=5, the reference's default: the k=5 counterpart of the whole-net tests of
tests/test_gpu_recurrent.py, whose helpers it imports.  tests/unet_ref.py is restated at kernel_size=5 for the duration of this
module (and put back), on the seeds of tests/golden/unet_k5_small.npz -- the fixture tests/test_conv5x5_host.py holds the
restatement to, with every ReLU pre-activation >= 1e-5 away from zero.

fp32 mode: outputs, final states and every parameter gradient of two carried calls within max(4 e32, 4 * 2^-23) of the float64
restatement (`_measure` of tests/test_gpu_recurrent.py); bf16x3 mode (the 5x5 layers run exact fp32, the 3x3 cells and residual
blocks split precision): its fixed 1e-3.  Under EBFI_STRICT_NATIVE=1 forward and backward run without a convolution leaving the
native kernels; two runs give the same bits; a captured two-call step replays the eager bits.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_recurrent as T  # noqa: E402
import unet_ref as R  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd import conv  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def k5_cases():
    """case -> (seed, xs, cots, float64 run, float32 run) of the restatement at kernel_size=5 on the k=5 fixture's seeds: computed
    once, shared.  The restatement's configuration stays patched for the module's tests and is restored after the last."""
    before = R.CFG["kernel_size"]
    R.CFG["kernel_size"] = 5
    try:
        fixture = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_k5_small.npz"))
        out = {}
        for i, case in enumerate(R.CASES):
            seed = int(fixture["seeds"][i])
            xs, cots = R.make_inputs(seed + 1000, case)
            state = R.fill_state(seed, case)
            out[case] = (seed, xs, cots, R.run(case, state, xs, cots), R.run(case, state, xs, cots, dtype=torch.float32))
        yield out
    finally:
        R.CFG["kernel_size"] = before


def _is_k5(net):
    return net.head.conv2d.weight.shape[-1] == 5 and net.encoders[0].conv.conv2d.weight.shape[-1] == 5 and \
        net.decoders[0].conv2d.weight.shape[-1] == 5


@pytest.mark.parametrize("case", list(R.CASES))
def test_whole_net_k5_fp32_against_float64(k5_cases, case):
    seed, xs, cots, ref64, ref32 = k5_cases[case]
    assert conv.get_compute_dtype() == "fp32" and _is_k5(T._net(case, seed))
    names, got = T._device_run(case, seed, xs, cots)
    failures = T._compare("net k5 %s fp32" % case, names, got, ref64, ref32)
    assert not failures, failures


@pytest.mark.parametrize("case", list(R.CASES))
def test_whole_net_k5_bf16x3_against_float64(k5_cases, case):
    seed, xs, cots, ref64, ref32 = k5_cases[case]
    before = conv.get_compute_dtype()
    conv.set_compute_dtype("bf16x3")
    try:
        names, got = T._device_run(case, seed, xs, cots)
    finally:
        conv.set_compute_dtype(before)
    failures = T._compare("net k5 %s bf16x3" % case, names, got, ref64, ref32, fixed=1e-3)
    assert not failures, failures


@pytest.mark.parametrize("case", ["A", "B", "D", "E"])
def test_strict_native_forward_and_backward_at_k5(k5_cases, case, monkeypatch, capfd):
    """kernel_size=5, norm=None, use_upsample_conv=True: no convolution leaves the native kernels, and none is reported."""
    monkeypatch.setenv("EBFI_STRICT_NATIVE", "1")
    seed, xs, cots, _, _ = k5_cases[case]
    _, (outs, states, grads) = T._device_run(case, seed, xs, cots)
    assert all(torch.isfinite(t).all() for t in outs + states + grads)
    assert "runs on torch" not in capfd.readouterr().err


def test_pad_5_still_raises_under_the_strict_switch(monkeypatch):
    from ebfi_amd.model import ConvLayer
    monkeypatch.setenv("EBFI_STRICT_NATIVE", "1")
    layer = ConvLayer(4, 4, 5, stride=2, padding=5).cuda()
    with pytest.raises(N.EbfiNativeError, match="EBFI_STRICT_NATIVE"):
        layer(torch.zeros(1, 4, 8, 8, device="cuda"))
    # ... and pad 4 does not
    assert ConvLayer(4, 4, 5, stride=2, padding=4).cuda()(torch.zeros(1, 4, 8, 8, device="cuda")).shape == (1, 4, 6, 6)


def test_two_k5_runs_give_the_same_bits(k5_cases):
    seed, xs, cots, _, _ = k5_cases["A"]
    names = [n for n, _ in R.names_and_shapes("A")]
    net = T._net("A", seed)
    assert _is_k5(net)
    xd, cd = [x.float().cuda() for x in xs], [c.float().cuda() for c in cots]
    first, second = T._bits(T._two_calls(net, xd, cd, names)), T._bits(T._two_calls(net, xd, cd, names))
    assert first == second and len(first) == 2 + 4 + len(names)


def test_captured_two_call_k5_step_replays_the_eager_bits(k5_cases):
    seed, xs, cots, _, _ = k5_cases["A"]
    names = [n for n, _ in R.names_and_shapes("A")]
    net = T._net("A", seed)
    xd, cd = [x.float().cuda() for x in xs], [c.float().cuda() for c in cots]
    eager = T._bits(T._two_calls(net, xd, cd, names))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        T._two_calls(net, xd, cd, names)                        # (the eager pass a capture runs first)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = T._two_calls(net, xd, cd, names)
    for _ in range(2):
        for t in captured[0] + captured[1] + captured[2]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert T._bits(captured) == eager
