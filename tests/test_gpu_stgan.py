"""The STGAN adversarial loss on the device (csrc/stgan.hip, ebfi_amd.gan): BatchNorm + LeakyReLU, Adamax, the whole
Adversarial call against the reference's own float64 numbers (tests/golden/stgan_small.npz), reproducibility, the Engine hook.

Accuracy bars are MEASURED, not fixed: for every output, e = max |x - x64| / max |x64| against float64; the yardstick e32 is the
same figure for the same law run in float32 on the CPU (torch's own batch_norm + leaky_relu and its autograd for the layer,
tests/stgan_ref.py in float32 for the whole call); pass when e <= max(4 e32, 4 float32 ulps of the output scale).  The factor 4
is because only the order of the sums differs.  Every figure is printed (pytest -s); profiles/stgan.md holds a run's."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stgan_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR, ULP = 4.0, 2.0 ** -23
SLOPE, EPS, MOMENTUM = 0.2, 1e-5, 0.1
SMALL = dict(step=2, channels=[8, 8, 16, 16])            # (the engine tests' small model, tests/test_gpu_validation.py)


def _rel(x, x64):
    x64 = torch.as_tensor(x64, dtype=torch.float64).reshape(-1)
    x = torch.as_tensor(x).detach().double().cpu().reshape(-1)
    scale = float(x64.abs().max())
    return float((x - x64).abs().max()) / scale if scale > 0 else float((x - x64).abs().max())


def _held(tag, key, got, want64, yard32, failures):
    e, e32 = _rel(got, want64), _rel(yard32, want64)
    bar = max(FACTOR * e32, FACTOR * ULP)
    print("stgan-accuracy %-28s %-12s e=%.3e e32=%.3e bar=%.3e" % (tag, key, e, e32, bar))
    if not e <= bar:
        failures.append((tag, key, e, e32))


# ------------------------------------------------------------------ BatchNorm + LeakyReLU
BN_CASES = [((3, 8, 5, 7), 0.0, 1.0), ((2, 64, 2, 2), 0.0, 1.0), ((1, 16, 33, 4), 0.0, 1.0), ((3, 8, 5, 7), 100.0, 0.1)]
BN_IDS = ["3x8x5x7", "2x64x2x2", "1x16x33x4", "3x8x5x7_mean100_spread0.1"]


def _bn_native(x, gamma, beta, dy=None, running=None):
    """-> (y, stats) or, with dy, (y, dx, dgamma, dbeta).  running = (rm, rv, nbt) device tensors, updated in place."""
    from ebfi_amd import _native as N
    lib = N.lib()
    B, C, H, W = x.shape
    dev = x.device
    y, stats = torch.empty_like(x), torch.empty(C, 2, dtype=torch.float64, device=dev)
    need = int(lib.ebfi_bn_lrelu_workspace(B, C, H * W))
    assert need == -(-B * H * W // 4096) * C * 16
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    rm, rv, nbt = running if running is not None else (None, None, None)
    st = N.stream_ptr(dev)
    N.check(lib.ebfi_bn_lrelu_forward(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), N.ptr(stats), N.ptr(rm), N.ptr(rv), N.ptr(nbt), B, C,
                                      H * W, EPS, MOMENTUM, SLOPE, N.ptr(ws), need, st), "ebfi_bn_lrelu_forward")
    if dy is None:
        return y, stats
    dx, dg, db = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
    N.check(lib.ebfi_bn_lrelu_backward(N.ptr(dy), N.ptr(x), N.ptr(y), N.ptr(gamma), N.ptr(stats), N.ptr(dx), N.ptr(dg), N.ptr(db), B, C,
                                       H * W, SLOPE, N.ptr(ws), need, st), "ebfi_bn_lrelu_backward")
    dx2 = torch.empty_like(x)                          # the generator's form: no parameter gradient
    N.check(lib.ebfi_bn_lrelu_backward(N.ptr(dy), N.ptr(x), N.ptr(y), N.ptr(gamma), N.ptr(stats), N.ptr(dx2), N.ptr(None), N.ptr(None),
                                       B, C, H * W, SLOPE, N.ptr(ws), need, st), "ebfi_bn_lrelu_backward")
    assert torch.equal(dx, dx2)
    return y, dx, dg, db


def _bn_torch(x, gamma, beta, dy, dtype):
    x, gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    y = F.leaky_relu(F.batch_norm(x, None, None, gamma, beta, True, MOMENTUM, EPS), SLOPE)
    y.backward(dy.to(dtype))
    return y.detach(), x.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("shape,mean,spread", BN_CASES, ids=BN_IDS)
def test_bn_lrelu_forward_and_backward_within_four_times_torch_float32(shape, mean, spread):
    g = torch.Generator().manual_seed(sum(shape) + int(mean))
    x = torch.randn(shape, generator=g) * spread + mean
    C = shape[1]
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(shape, generator=g)
    want = _bn_torch(x, gamma, beta, dy, torch.float64)
    yard = _bn_torch(x, gamma, beta, dy, torch.float32)
    got = _bn_native(x.cuda(), gamma.cuda(), beta.cuda(), dy.cuda())
    torch.cuda.synchronize()
    failures = []
    for key, a, b, c in zip(("y", "dx", "dgamma", "dbeta"), got, want, yard):
        _held("bn_lrelu " + "x".join(map(str, shape)) + (" m100" if mean else ""), key, a, b, c, failures)
    assert not failures, failures
    if mean:                                  # the variance survived: y has the spread of a normalised plane, not rounding noise
        assert 0.5 < float(got[0].std()) < 2.0


def test_bn_running_statistics_after_three_passes_follow_the_law():
    shape = (3, 8, 5, 7)
    g = torch.Generator().manual_seed(5)
    C, n = shape[1], shape[0] * shape[2] * shape[3]
    gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
    rm, rv, nbt = torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.zeros((), dtype=torch.int64).cuda()
    rm64, rv64 = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    for k in range(3):
        x = torch.randn(shape, generator=g) * (1 + k) + 3 * k
        _bn_native(x.cuda(), gamma, beta, running=(rm, rv, nbt))
        x64 = x.double()
        mean, var = x64.mean((0, 2, 3)), x64.var((0, 2, 3), unbiased=False)
        rm64 = 0.9 * rm64 + 0.1 * mean
        rv64 = 0.9 * rv64 + 0.1 * var * n / (n - 1)
    torch.cuda.synchronize()
    assert int(nbt) == 3
    # float32 storage, rounded once per pass: 4 ulps of the scale
    assert _rel(rm, rm64) <= 4 * ULP and _rel(rv, rv64) <= 4 * ULP, (_rel(rm, rm64), _rel(rv, rv64))


# ------------------------------------------------------------------ temporal input, BCE
def test_temporal_input_and_its_adjoint_and_the_bce_pair():
    from ebfi_amd import _native as N
    from ebfi_amd.gan import bce_logits_pair
    lib = N.lib()
    g = torch.Generator().manual_seed(3)
    for B, H, W in ((2, 5, 7), (3, 4, 4)):                 # a scalar tail (C*H*W = 105) and the 16-byte form
        frames = torch.rand(B, 2, 3, H, W, generator=g).cuda()
        f1 = torch.rand(B, 3, H, W, generator=g).cuda()
        out = torch.empty(B, 6, H, W, device="cuda")
        f0, f2 = frames[:, 0], frames[:, 1]
        N.check(lib.ebfi_stgan_temporal_forward(N.ptr(f0), f0.stride(0), N.ptr(f1), f1.stride(0), N.ptr(f2), f2.stride(0), N.ptr(out), B,
                                                3 * H * W, N.stream_ptr(out.device)), "temporal_forward")
        assert torch.equal(out, torch.cat([f1 - f0, f1 - f2], 1))
        gt, gs = torch.randn(B, 6, H, W, generator=g).cuda(), torch.randn(B, 3, H, W, generator=g).cuda()
        gf = torch.empty(B, 3, H, W, device="cuda")
        N.check(lib.ebfi_stgan_temporal_backward(N.ptr(gt), N.ptr(gs), N.ptr(gf), B, 3 * H * W, N.stream_ptr(gf.device)), "temporal_backward")
        assert torch.equal(gf, gt[:, :3] + gt[:, 3:] + gs)
    # BCE with logits, at moderate and at saturating logits (the stable form: no overflow, no log(0))
    xf = torch.tensor([[-40.0], [-1.5], [0.0], [0.3], [90.0]])
    xr = torch.tensor([[120.0], [2.5], [0.0], [-0.7], [-60.0]])
    loss, gf, gr = bce_logits_pair(xf.cuda(), xr.cuda())
    a, b = xf.double().requires_grad_(True), xr.double().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(a, torch.zeros_like(a)) + F.binary_cross_entropy_with_logits(b, torch.ones_like(b))
    want.backward()
    assert abs(float(loss) - float(want)) <= 4 * ULP * float(want)
    assert _rel(gf, a.grad) <= 4 * ULP and _rel(gr, b.grad) <= 4 * ULP
    only_g, none_f, g_g = bce_logits_pair(None, xr.cuda())
    assert none_f is None and abs(float(only_g) - float(F.binary_cross_entropy_with_logits(xr.double(), torch.ones(5, 1, dtype=torch.float64)))) <= 4 * ULP * float(only_g)
    assert torch.equal(g_g, gr)


# ------------------------------------------------------------------ the classifier's linear layers
LINEAR_CASES = [(3, 512, 1024), (2, 1152, 1024), (9, 1024, 1), (2, 7, 5)]      # P = 32 | P = 48 | the head, two row chunks | scalar path


@pytest.mark.parametrize("B,K,n_out", LINEAR_CASES, ids=["3x512x1024", "2x1152x1024", "9x1024x1", "2x7x5"])
def test_linear_layers_within_four_times_torch_float32(B, K, n_out):
    from ebfi_amd import _native as N
    lib = N.lib()
    g = torch.Generator().manual_seed(B + K + n_out)
    x, w, b = torch.randn(B, K, generator=g), torch.randn(n_out, K, generator=g) / K ** 0.5, torch.randn(n_out, generator=g)
    gy = torch.randn(B, n_out, generator=g)

    def ref(dtype):
        xx, ww, bb = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
        y = F.leaky_relu(F.linear(xx, ww, bb), SLOPE)
        y.backward(gy.to(dtype))
        return y.detach(), xx.grad, ww.grad, bb.grad

    want, yard = ref(torch.float64), ref(torch.float32)
    xd, wd, bd, gyd = x.cuda(), w.cuda(), b.cuda(), gy.cuda()
    y, gx, gw, gb = torch.empty(B, n_out).cuda(), torch.empty(B, K).cuda(), torch.empty(n_out, K).cuda(), torch.empty(n_out).cuda()
    st = N.stream_ptr(xd.device)
    N.check(lib.ebfi_linear_forward(N.ptr(xd), N.ptr(wd), N.ptr(bd), N.ptr(y), B, K, n_out, 1, SLOPE, st), "ebfi_linear_forward")
    # the gradient of the pre-activation: grad_y through LeakyReLU'(y), as the layer above's data gradient delivers it
    gpre = gyd * torch.where(y > 0, 1.0, SLOPE)
    N.check(lib.ebfi_linear_backward_data(N.ptr(gpre), N.ptr(wd), N.ptr(None), SLOPE, N.ptr(gx), B, K, n_out, st), "ebfi_linear_backward_data")
    N.check(lib.ebfi_linear_backward_weight(N.ptr(gpre), N.ptr(xd), N.ptr(gw), N.ptr(gb), B, K, n_out, st), "ebfi_linear_backward_weight")
    # the mask form: grad_x times LeakyReLU'(mask) in the same launch
    mask = torch.randn(B, K, generator=g).cuda()
    gxm = torch.empty_like(gx)
    N.check(lib.ebfi_linear_backward_data(N.ptr(gpre), N.ptr(wd), N.ptr(mask), SLOPE, N.ptr(gxm), B, K, n_out, st), "ebfi_linear_backward_data")
    torch.cuda.synchronize()
    assert torch.equal(gxm, torch.where(mask > 0, gx, gx * torch.tensor(SLOPE, dtype=torch.float32).cuda()))
    failures = []
    for key, a, c, d in zip(("y", "dx", "dweight", "dbias"), (y, gx, gw, gb), want, yard):
        _held("linear %dx%dx%d" % (B, K, n_out), key, a, c, d, failures)
    assert not failures, failures


# ------------------------------------------------------------------ Adamax
def _adamax_data(n, steps, seed):
    """As tests/test_gpu_optim.py: parameters N(0,1) exp(U(-6,1)); gradients N(0,1) exp(U(-12,2)), every fifth element zero."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * torch.exp(torch.rand(n, generator=g) * 7 - 6)
    grads = []
    for _ in range(steps):
        x = torch.randn(n, generator=g) * torch.exp(torch.rand(n, generator=g) * 14 - 12)
        x[2::5] = 0.0
        grads.append(x)
    return p, grads


def _adamax_torch(p0, grads, dtype, lrs, wd):
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.Adamax([p], lr=lrs[0], betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        p.grad = g.to(dtype)
        opt.step()
    return {"param": p.detach(), "exp_avg": opt.state[p]["exp_avg"], "exp_inf": opt.state[p]["exp_inf"]}


@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["wd0", "wd0.01"])
def test_adamax_within_four_times_torch_float32_error(wd):
    """n = 1003: 250 quads and a scalar tail of three; five steps, the lr halved before the third (it travels by value).  Held to
    torch.optim.Adamax as tests/test_gpu_optim.py holds the other kinds: e = max |x - x64| / max(|x64|, lr) <= 4 e32."""
    from ebfi_amd import _native as N
    lib = N.lib()
    n, steps, lr0 = 1003, 5, 1e-2
    lrs = [lr0 if s < 2 else lr0 / 2 for s in range(steps)]
    p0, grads = _adamax_data(n, steps, 2003)
    p, m, u = p0.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    p_split, m_split, u_split = p.clone(), m.clone(), u.clone()
    step = torch.zeros((), device="cuda")
    for g, lr in zip(grads, lrs):
        step += 1
        gd = g.cuda()
        N.check(lib.ebfi_adamax_step(N.ptr(p), N.ptr(gd), N.ptr(None), N.ptr(m), N.ptr(u), N.ptr(step), n, lr, 0.9, 0.999, 1e-8, wd,
                                     N.stream_ptr(p.device)), "ebfi_adamax_step")
        # the two-buffer form: g = ga + gb exactly (gb holds every other element, ga the rest)
        ga, gb = gd.clone(), torch.zeros_like(gd)
        gb[::2], ga[::2] = gd[::2], 0.0
        N.check(lib.ebfi_adamax_step(N.ptr(p_split), N.ptr(ga), N.ptr(gb), N.ptr(m_split), N.ptr(u_split), N.ptr(step), n, lr, 0.9, 0.999,
                                     1e-8, wd, N.stream_ptr(p.device)), "ebfi_adamax_step")
    torch.cuda.synchronize()
    assert torch.equal(p, p_split) and torch.equal(m, m_split) and torch.equal(u, u_split)
    got = {"param": p, "exp_avg": m, "exp_inf": u}
    ref64, ref32 = _adamax_torch(p0, grads, torch.float64, lrs, wd), _adamax_torch(p0, grads, torch.float32, lrs, wd)
    err = lambda x, x64: float(((x.double().cpu() - x64).abs() / x64.abs().clamp_min(lrs[-1])).max())
    worst = {}
    for key in got:
        e, e32 = err(got[key], ref64[key]), err(ref32[key], ref64[key])
        print("stgan-accuracy adamax wd=%g %-8s e=%.3e e32=%.3e" % (wd, key, e, e32))
        if not e <= FACTOR * e32:
            worst[key] = (e, e32)
    assert not worst, worst
    assert not torch.equal(p.cpu(), p0)


# ------------------------------------------------------------------ the whole Adversarial
@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "stgan_small.npz"))


def _native_adversarial(P, state):
    from ebfi_amd.gan import Adversarial
    adv = Adversarial(P, "STGAN")
    adv.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in state.items()})
    adv = adv.cuda()
    assert adv.discriminator.views_intact()
    return adv


def _summary(state, names):
    """What the fixture keeps of a state: parameter sums, their first 8 elements, the running statistics, the counters."""
    pn = [n for n in names if R.is_parameter(n)]
    st = {k: v.detach().cpu() for k, v in state.items()}
    heads = torch.zeros(len(pn), 8, dtype=torch.float64)
    for i, n in enumerate(pn):
        h = st[n].double().reshape(-1)[:8]
        heads[i, :h.numel()] = h
    return {"sums": torch.stack([st[n].double().sum() for n in pn]), "heads": heads,
            "run": torch.cat([st[n].double().reshape(-1) for n in names if n.endswith("running_mean")] +
                             [st[n].double().reshape(-1) for n in names if n.endswith("running_var")]),
            "tracked": torch.stack([st[n] for n in names if n.endswith("num_batches_tracked")])}


def _native_call(adv, fake, real, frames):
    fake = fake.cuda().requires_grad_(True)
    loss_g = adv(fake, real.cuda(), frames.cuda())
    assert loss_g.dim() == 0 and loss_g.requires_grad and adv.loss_d.is_cuda
    (g,) = torch.autograd.grad(loss_g, fake)
    return adv.loss_d.clone(), loss_g.detach().clone(), g


def test_two_calls_against_the_reference_fixture(fixture):
    """P = 32, B = 3, two consecutive calls from fill_state(20, 32), against the reference's own float64 numbers.  Yardstick: the
    restatement in float32 on the CPU.  The inputs were chosen (tests/golden/make_stgan_golden.py) so that this yardstick flips
    no LeakyReLU mask at all -- asserted below -- with the smallest pre-activation an order of magnitude above its error."""
    names = [str(n) for n in fixture["names"]]
    assert names == [n for n, _ in R.names_and_shapes(32)]
    state = R.fill_state(20, 32)
    adv = _native_adversarial(32, state)
    assert list(adv.state_dict()) == names
    ref64, yard = R.RefAdversarial(32, state), R.RefAdversarial(32, state, torch.float32)
    ref64.preacts, yard.preacts = [], []
    failures = []
    for c in range(2):
        fake, real, frames = (R.inputs_from_bytes(fixture[k][c]) for k in ("fake_u8", "real_u8", "frames_u8"))
        ld, lg, g = _native_call(adv, fake, real, frames)
        yd, yg, ygrad = yard.call(fake, real, frames)
        ref64.call(fake, real, frames)
        torch.cuda.synchronize()
        got, y32 = _summary(adv.state_dict(), names), _summary(yard.state, names)
        tag = "adversarial P32 B3 call %d" % c
        _held(tag, "loss_d", ld, fixture["loss_d"][c], yd, failures)
        _held(tag, "loss_g", lg, fixture["loss_g"][c], yg, failures)
        _held(tag, "grad_fake", g, fixture["grad_fake"][c], ygrad, failures)
        _held(tag, "param_sums", got["sums"], fixture["param_sums"][c], y32["sums"], failures)
        _held(tag, "param_heads", got["heads"], fixture["param_heads"][c], y32["heads"], failures)
        _held(tag, "running", got["run"], fixture["running"][c], y32["run"], failures)
        assert got["tracked"].tolist() == fixture["tracked"][c].tolist() == [3 * (c + 1)] * 16
        assert adv.loss == pytest.approx(float(ld)) and isinstance(adv.loss, float)
    flips = [(float(a[(a > 0) != (b > 0)].abs().max())) for a, b in zip(ref64.preacts, yard.preacts) if bool(((a > 0) != (b > 0)).any())]
    assert not flips, "the float32 yardstick flips LeakyReLU masks on this input (largest pre-activation %.1e)" % max(flips)
    assert not failures, failures
    assert float(adv.optimizer.inner.state[adv.optimizer.flat]["step"]) == 2 and adv.discriminator.views_intact()


def test_odd_maps_against_the_restatement():
    """P = 48, B = 2 (q = 3: 3 x 3 maps at the bottom, odd rows everywhere below 48), one call, against tests/stgan_ref.py alone.
    Input seed 53: of the seeds 48 .. 59 the one whose smallest pre-activation (3.9e-6) stands furthest above the float32
    yardstick's error in its layer (checked on the CPU); the yardstick flips no mask (asserted)."""
    P, B = 48, 2
    state = R.fill_state(7, P)
    (fake_u8, real_u8, frames_u8), = R.make_inputs(53, B, P, 1)
    fake, real, frames = (R.inputs_from_bytes(a) for a in (fake_u8, real_u8, frames_u8))
    names = [n for n, _ in R.names_and_shapes(P)]
    adv = _native_adversarial(P, state)
    ref64, yard = R.RefAdversarial(P, state), R.RefAdversarial(P, state, torch.float32)
    ref64.preacts, yard.preacts = [], []
    ld, lg, g = _native_call(adv, fake, real, frames)
    wd, wg, wgrad = ref64.call(fake, real, frames)
    yd, yg, ygrad = yard.call(fake, real, frames)
    torch.cuda.synchronize()
    flips = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(ref64.preacts, yard.preacts))
    assert flips == 0, "the float32 yardstick flips %d LeakyReLU masks on this input: it proves nothing" % flips
    got, want, y32 = _summary(adv.state_dict(), names), _summary(ref64.state, names), _summary(yard.state, names)
    failures = []
    tag = "adversarial P48 B2"
    for key, a, b, c in (("loss_d", ld, wd, yd), ("loss_g", lg, wg, yg), ("grad_fake", g, wgrad, ygrad), ("param_sums", got["sums"], want["sums"], y32["sums"]),
                         ("param_heads", got["heads"], want["heads"], y32["heads"]), ("running", got["run"], want["run"], y32["run"])):
        _held(tag, key, a, b, c, failures)
    assert not failures, failures


def test_two_runs_from_the_same_state_give_the_same_bits(fixture):
    state = R.fill_state(20, 32)
    runs = []
    for _ in range(2):
        adv = _native_adversarial(32, state)
        out = []
        for c in range(2):
            out += list(_native_call(adv, *(R.inputs_from_bytes(fixture[k][c]) for k in ("fake_u8", "real_u8", "frames_u8"))))
        torch.cuda.synchronize()
        runs.append(out + [adv.discriminator.flat.clone()] + [b.clone() for b in adv.discriminator.buffers()])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))


def test_refusals_happen_before_any_device_work():
    from ebfi_amd.gan import Adversarial
    adv = Adversarial(16).cuda()
    x = torch.rand(1, 3, 16, 16, device="cuda")
    with pytest.raises(ValueError, match="more than 1 value"):
        adv(x, x, torch.rand(1, 2, 3, 16, 16, device="cuda"))          # n == 1 at the last stage
    x2 = torch.rand(2, 3, 16, 32, device="cuda")
    with pytest.raises(ValueError, match="PatchSize"):
        adv(x2, x2, torch.rand(2, 2, 3, 16, 32, device="cuda"))        # H != W == P
    assert float(adv.discriminator.s_features[0][1].num_batches_tracked) == 0
    x3 = torch.rand(2, 3, 16, 16, device="cuda")                       # ... and P = 16 with B = 2 runs
    assert torch.isfinite(adv(x3, x3 * 0.9, torch.rand(2, 2, 3, 16, 16, device="cuda")))


# ------------------------------------------------------------------ the Engine hook
def _term(weight=0.05, seed=3):
    from ebfi_amd.gan import Adversarial, AdversarialTerm
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    adv = Adversarial(32, "STGAN")
    torch.random.set_rng_state(state)
    return AdversarialTerm(adv, weight)


def _engine(**kw):
    from ebfi_amd.engine import Engine
    return Engine(SMALL, device="cuda", precision="bf16x3", lr=1e-3, seed=7, **kw)


def _batch(seed, neighbours=True):
    from ebfi_amd.engine import synthetic_batch
    batch = synthetic_batch(2, 32, 32, device="cuda", seed=seed)
    if not neighbours:
        return batch
    g = torch.Generator().manual_seed(seed + 31337)
    return batch + (torch.rand(2, 2, 3, 32, 32, generator=g).cuda(),)


def test_engine_steps_with_the_term_eager_and_captured_give_the_same_bits():
    """32 x 32: the smallest crop of the existing engine tests that is a multiple of 16.  Four steps: the two eager calibration
    steps of the fp16 backward, the capture (whose warm-up passes must not count as discriminator steps), one more replay.
    Whenever the two engines enter a step with bit-equal model weights -- always up to and including the captured step -- the
    step's loss, loss_d, every discriminator parameter, its running statistics and its Adamax state must agree to the bit.
    The MODEL's gradient of a captured step agrees with an eager one's to rounding only, with or without the term (the pair of
    engines without it is run alongside and held to the same rule; cf. the bounds of test_gpu_lpips_alex_grad.py::
    test_engine_graph_step_with_the_alex_term_equals_the_eager_one): from then on the discriminator sees different frames and
    the comparison is the existing test's, to rounding."""
    engines = [_engine(adversarial=_term(), graph=g, strict_graph=g) for g in (False, True)]
    plain = [_engine(graph=g, strict_graph=g) for g in (False, True)]
    d0 = engines[0].adversarial.discriminator.flat.clone()
    a, b = (e.adversarial for e in engines)
    held = []
    for it in range(4):
        batch = _batch(100 + it)
        same_in = torch.equal(engines[0].optimizer.flat.detach(), engines[1].optimizer.flat.detach())
        plain_in = torch.equal(plain[0].optimizer.flat.detach(), plain[1].optimizer.flat.detach())
        losses = [e.train_step(*batch).clone() for e in engines]
        plain_losses = [e.train_step(*batch[:5]).clone() for e in plain]
        torch.cuda.synchronize()
        ld = [float(e.adversarial.loss_d) for e in engines]
        print("stgan-engine step %d: model weights bit-equal on entry: with the term %s, without %s; loss_d %r" % (it, same_in, plain_in, ld))
        assert ld[0] > 0 and (not plain_in or torch.equal(*plain_losses))
        if same_in:
            held.append(it)
            assert torch.equal(losses[0], losses[1]), (it, losses)
            assert torch.equal(a.loss_d, b.loss_d), (it, ld)
            assert torch.equal(a.discriminator.flat, b.discriminator.flat), it
            assert all(torch.equal(x, y) for x, y in zip(a.discriminator.buffers(), b.discriminator.buffers())), it
        else:
            assert not plain_in or it > held[-1] + 1, "the term made a step diverge that the engine alone repeats to the bit"
            assert torch.allclose(losses[0], losses[1], rtol=1e-5, atol=0), (it, losses)
            assert torch.allclose(a.loss_d, b.loss_d, rtol=1e-4, atol=0), (it, ld)
            assert torch.allclose(a.discriminator.flat, b.discriminator.flat, rtol=1e-3, atol=1e-5), it
        if it == 0:                               # the model's packed gradient differs from a run without the term
            assert not torch.equal(engines[0].bucket.flat, plain[0].bucket.flat) and torch.isfinite(engines[0].bucket.flat).all()
    assert held[:3] == [0, 1, 2]                  # ... the captured step among them
    assert len(engines[1]._graphs) == 1 and not engines[1].graph_capture_failed and engines[1].use_graph
    assert not torch.equal(a.discriminator.flat, d0)
    sa, sb = (x.optimizer.inner.state[x.optimizer.flat] for x in (a, b))
    assert float(sa["step"]) == float(sb["step"]) == 4
    assert int(a.discriminator.t_features[7][1].num_batches_tracked) == int(b.discriminator.t_features[7][1].num_batches_tracked) == 12
    # where the engine alone repeats its weights to the bit under capture, so must the engine with the term
    if torch.equal(plain[0].optimizer.flat.detach(), plain[1].optimizer.flat.detach()):
        assert torch.equal(engines[0].optimizer.flat.detach(), engines[1].optimizer.flat.detach())
        assert torch.equal(a.discriminator.flat, b.discriminator.flat) and torch.equal(sa["exp_inf"], sb["exp_inf"])
    for (n, p), q in zip(engines[0].model.named_parameters(), engines[1].model.parameters()):
        assert torch.allclose(p, q, rtol=1e-3, atol=1e-5), (n, float((p - q).abs().max()))
    # the discriminator is no part of the model
    assert engines[0].bucket.numel == plain[0].bucket.numel and set(engines[0].model.state_dict()) == set(plain[0].model.state_dict())
    with pytest.raises(ValueError, match="sixth input"):
        engines[0].train_step(*_batch(1, neighbours=False))
    with pytest.raises(ValueError, match="sixth input"):
        plain[0].train_step(*_batch(1))


def test_checkpoint_round_trip_restores_the_gan_key(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "ebfi-be_amd"))
    import train_ours as T
    config = {"model": {"name": "EVFIAutoEx", "args": SMALL}, "optimizer": {"name": "Adam", "args": {"lr": 1e-3}}}
    eng = _engine(adversarial=_term())
    for it in range(2):
        eng.train_step(*_batch(200 + it))
    path = T.save_checkpoint(str(tmp_path / "a" / "checkpoint-iteration1.pth"), eng, None, config, 1)[0]
    cpt = torch.load(path, map_location="cpu", weights_only=False)
    assert set(cpt) == set(T.CHECKPOINT_KEYS) | {"gan"}
    gan = cpt["gan"]
    assert gan["type"] == "STGAN" and gan["patch"] == 32 and len(gan["discriminator"]) == 100
    assert list(gan["discriminator"]) == [n[len(R.PREFIX):] for n, _ in R.names_and_shapes(32)]
    # torch's per-parameter layout: a torch.optim.Adamax over as many parameters loads it
    probe = torch.optim.Adamax([torch.nn.Parameter(torch.zeros_like(p, device="cpu")) for p in eng.adversarial.discriminator.parameters()])
    probe.load_state_dict(gan["optimizer"])
    assert len(gan["optimizer"]["state"]) == 52 and float(gan["optimizer"]["state"][0]["step"]) == 2
    again = _engine(adversarial=_term(seed=9))
    assert not torch.equal(again.adversarial.discriminator.flat, eng.adversarial.discriminator.flat)
    assert T.resume_checkpoint(path, again, None, config, map_location="cuda") == 2
    a, b = eng.adversarial, again.adversarial
    assert torch.equal(a.discriminator.flat, b.discriminator.flat) and b.discriminator.views_intact()
    assert all(torch.equal(x, y) for x, y in zip(a.discriminator.buffers(), b.discriminator.buffers()))
    sa, sb = (x.optimizer.inner.state[x.optimizer.flat] for x in (a, b))
    assert all(torch.equal(sa[k], sb[k]) for k in ("step", "exp_avg", "exp_inf"))
    # the next discriminator step is the one the first run takes (the Adamax state came along)
    g = torch.Generator().manual_seed(300)
    fake, real, frames = (torch.rand(s, generator=g).cuda() for s in ((2, 3, 32, 32), (2, 3, 32, 32), (2, 2, 3, 32, 32)))
    assert torch.equal(a(fake, real, frames), b(fake, real, frames)) and torch.equal(a.loss_d, b.loss_d)
    assert torch.equal(a.discriminator.flat, b.discriminator.flat)
    # --reset does not restore it; and an engine without the term writes the five keys it always wrote
    fresh = _engine(adversarial=_term(seed=9))
    keep = fresh.adversarial.discriminator.flat.clone()
    assert T.resume_checkpoint(path, fresh, None, config, reset=True, map_location="cuda") == 0
    assert torch.equal(fresh.adversarial.discriminator.flat, keep) and not fresh.adversarial.optimizer.inner.state
    plain = _engine()
    assert plain.adversarial is None
    plain.train_step(*_batch(400, neighbours=False))
    old = T.save_checkpoint(str(tmp_path / "b" / "checkpoint-iteration0.pth"), plain, None, config, 0)[0]
    assert tuple(torch.load(old, map_location="cpu", weights_only=False)) == T.CHECKPOINT_KEYS


def test_train_ours_with_gan_weight_runs_on_recorded_clips(tmp_path):
    """`train_ours.py --gan_weight W --data <dir>`: what this test is about is the command line -- the option turns
    dataset.NeedNeighborGT on, the device loader delivers the neighbours, the log line names the term and shows loss_d, and the
    checkpoint gains the `gan` key.  Three optimiser steps of a reduced-width model on two small synthetic clips."""
    import subprocess
    import yaml
    from ebfi_amd import clipdata
    root = os.path.dirname(HERE)
    for k in range(2):
        clipdata.write_synthetic_clip(str(tmp_path / ("clip%d.npz" % k)), num_imgs=17, H=32, W=32, events_per_frame=300, seed=k)
    cfg = yaml.safe_load(open(os.path.join(root, "ebfi-be_amd", "config", "train_ours.yml")))
    cfg["model"]["args"].update(FrameBasech=16, EventBasech=16, InterCH=16, TB=4, step=2, channels=[4, 4, 8, 8])
    cfg["trainer"].update(batch_size=2, height=32, width=32, output_path=str(tmp_path / "out"))
    cfg["train_dataloader"] = {"dataset": {"time_bins": 4, "NumFramePerPeriod": 4, "NumFramePerBlurry": 3, "ExposureMethod": "Fixed"}}
    cfg_path = str(tmp_path / "cfg.yml")
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    out = subprocess.run([sys.executable, os.path.join(root, "ebfi-be_amd", "train_ours.py"), "-c", cfg_path, "--data", str(tmp_path),
                          "--iterations", "3", "--gan_weight", "0.01", "-id", "gan"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Iteration: 2/3" in out.stdout and "(with 0.01 x STGAN)" in out.stdout and " loss_d: " in out.stdout and "saved" in out.stdout
    cpt = torch.load(str(tmp_path / "out" / "models" / cfg.get("experiment", "Ours") / "gan" / "checkpoint-iteration2.pth"),
                     map_location="cpu", weights_only=False)
    assert cpt["gan"]["patch"] == 32 and float(cpt["gan"]["optimizer"]["state"][0]["step"]) == 3
    assert cpt["config"]["train_dataloader"]["dataset"]["NeedNeighborGT"] is True
    assert int(cpt["gan"]["discriminator"]["s_features.0.1.num_batches_tracked"]) == 9
