"""ebfi_scalar_conv_backward spread over a grid of workgroups (csrc/fuse.hip): 64 (layer, channel) items of grad_weight /
grad_bias per workgroup, one workgroup per (sample, input) pair of grad_v.  Every size at which the grid changes shape -- one
item, exactly one workgroup of items (S*C = 64), a ragged last workgroup (C = 100), the largest bank (S = 32), one and several
pairs -- with and without a bias and with and without grad_v, against a float64 einsum at the tolerance of
tests/test_gpu_scalar_conv.py; two runs give the same bits."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

SLOPE = 0.01


def _run(v, ws, bs, g, want_gv):
    from ebfi_amd import fused
    vv = v.cuda().requires_grad_(want_gv)
    ww = [w.cuda().requires_grad_(True) for w in ws]
    bb = [None if b is None else b.cuda().requires_grad_(True) for b in bs]
    assert fused.scalar_conv_usable(vv, ww)
    out = fused.scalar_conv_bank(vv, ww, bb, SLOPE)
    out.backward(g.cuda())
    res = {"out": out.detach().cpu(), "gw": torch.stack([w.grad.cpu() for w in ww])}
    if bs[0] is not None:
        res["gb"] = torch.stack([b.grad.cpu() for b in bb])
    if want_gv:
        res["gv"] = vv.grad.cpu()
    else:
        assert vv.grad is None
    return res


@pytest.mark.parametrize("S,B,K,C", list(itertools.product((1, 12, 32), (1, 8), (1, 8), (1, 64, 100))))
def test_scalar_conv_backward_grid_matches_float64(S, B, K, C):
    torch.manual_seed(((S * 10 + B) * 10 + K) * 1000 + C)
    v = torch.randn(B, K)
    ws = [torch.randn(C, K, 1, 1) for _ in range(S)]
    g = torch.randn(S, B, C)
    w64 = torch.stack([w.flatten(1) for w in ws]).double()                                    # [S, C, K]
    for bias, want_gv in itertools.product((True, False), (True, False)):
        bs = [torch.randn(C) if bias else None for _ in range(S)]
        got = _run(v, ws, bs, g, want_gv)
        pre = torch.einsum("bk,sck->sbc", v.double(), w64)
        if bias:
            pre = pre + torch.stack(bs).double()[:, None, :]
        ref_out = torch.where(pre > 0, pre, pre * SLOPE)
        assert torch.allclose(got["out"].double(), ref_out, rtol=1e-5, atol=1e-5)
        # (the backward's mask is the sign of the saved forward output)
        gp = g.double() * torch.where(got["out"] > 0, 1.0, SLOPE).double()
        ref = {"gw": torch.einsum("sbc,bk->sck", gp, v.double()).reshape(S, C, K, 1, 1), "gb": gp.sum(1),
               "gv": torch.einsum("sbc,sck->bk", gp, w64)}
        for name, t in got.items():
            if name == "out":
                continue
            assert t.shape == ref[name].shape, name
            err = (t.double() - ref[name]).abs().max().item()
            print("S=%d B=%d K=%d C=%d bias=%d gv=%d %s: max err %.3e" % (S, B, K, C, bias, want_gv, name, err))
            assert torch.allclose(t.double(), ref[name], rtol=1e-5, atol=1e-5), (name, err)
        again = _run(v, ws, bs, g, want_gv)
        for name, t in got.items():
            assert torch.equal(t.view(torch.int32), again[name].view(torch.int32)), name
