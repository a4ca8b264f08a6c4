"""ebfi_amd.lpips.AlexLPIPSLoss.loss (ebfi_lpips_alex_forward_train / ebfi_lpips_alex_backward: the five tap adjoints with the
3x3/s2 pools' gather, the 3x3 data gradients, the 5x5 MFMA kernel, the 11x11 stride-4 kernel and its input epilogue) against the
float64 CPU autograd gradient of lpips_alex_grad_ref.

Error measure, per pair: max|got - want| / max|want| with want in float64, used where max|want| > 0 (a pair whose grad_out is 0
must come out exactly 0).  The bar follows the protocol of test_gpu_lpips_vgg_grad (profiles/lpips_vgg.md): a module fixture
evaluates the same cases by float32 autograd on the CPU, and the bar of a kind is 10 x that evaluation's worst error on the
kind's cases (the kernels sum K = 363 .. 4800 products in another order); the dead and the flat case are held to the random bar
and do not set it.  The float32 errors, the bars and the device errors are printed before they are asserted.  Every case uses
grad_out = (1.5, 0, -0.5)[:N].

Plus: an identical pair, the forward value against __call__, bit-reproducibility, NaN / Inf isolation per pair, no torch
convolution / pooling / ReLU on the path, a torch.cuda.graph capture, the perceptual_loss shim on two channels, and the Engine
hook."""
import pytest
import torch

from lpips_alex_grad_ref import CASES, case_id, grad_out_of, kind_of_bar, make_pair, pair_errors, ref_grad, trunk_of
from test_gpu_validation import SMALL
from test_lpips_host import write_weights

pytestmark = pytest.mark.gpu

FACTOR = 10.0
STRIDED = (3, 3, 71, 93, "random")


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    return write_weights(tmp_path_factory.mktemp("lpips_alex_grad"), seed=0)


@pytest.fixture(scope="module")
def alex(weights):
    from ebfi_amd.lpips import AlexLPIPSLoss, load_alex_lpips
    lin_path, backbone_path, _ = weights
    model = load_alex_lpips(lin_path, backbone_path, device="cuda", train=True)
    assert isinstance(model, AlexLPIPSLoss)
    return model


@pytest.fixture(scope="module")
def alex_dead():
    """The model of the dead case: conv1's bias lowered, so that flat regions give all-zero feature pixels."""
    from ebfi_amd.lpips import AlexLPIPSLoss
    dead = [c for c in CASES if c[4] == "dead"][0]
    return AlexLPIPSLoss(*trunk_of(dead), "cuda")


@pytest.fixture(scope="module")
def yardstick():
    """Per case (pred, target, normalize, grad_out, float64 gradient, float64 lpips) and per kind the bar: 10 x the worst error of
    the float32 CPU autograd gradient on the kind's cases.  Computed once; nothing below changes it."""
    cases, worst = {}, {}
    for case in CASES:
        ws, bs, heads = trunk_of(case)
        pred, target, normalize = make_pair(case)
        go = grad_out_of(case[0])
        want, lpips = ref_grad(pred, target, ws, bs, heads, go, normalize)
        f32, _ = ref_grad(pred, target, ws, bs, heads, go, normalize, dtype=torch.float32)
        assert torch.isfinite(want).all() and torch.isfinite(f32).all()
        errs = [e for e in pair_errors(f32, want) if e is not None]
        assert len(errs) == sum(1 for g in go if g != 0)
        cases[case] = (pred, target, normalize, go, want, lpips)
        if case[4] not in ("dead", "flat"):         # (held to the random bar; they do not set it)
            worst[kind_of_bar(case[4])] = max(worst.get(kind_of_bar(case[4]), 0.0), max(errs))
        print("lpips_alex_grad yardstick: %-28s float32-CPU error %s" % (case_id(case), " ".join("%.3e" % e for e in errs)))
    bars = {kind: FACTOR * v for kind, v in worst.items()}
    for kind in sorted(bars):
        print("lpips_alex_grad yardstick: kind %-9s float32-CPU worst error %.3e -> bar %.3e" % (kind, worst[kind], bars[kind]))
    assert set(bars) == {"random", "unclamped", "near"} and all(0 < b < 1e-2 for b in bars.values()), bars
    return cases, bars


def _grad(model, pred, target, go, normalize=True):
    """(lpips, d/dpred of sum_n go[n] lpips[n]) of the device loss; pred may be a view of a larger leaf."""
    if not pred.requires_grad:
        pred = pred.detach().requires_grad_(True)
    out = model.loss(pred, target, normalize=normalize)
    assert out.requires_grad and out.shape == (pred.shape[0],) and out.dtype == torch.float32
    (g,) = torch.autograd.grad(out, pred, go.to(out.device))
    assert g.shape == pred.shape and g.dtype == torch.float32
    return out.detach(), g


def _check(got, want, go, bar, label):
    errs = pair_errors(got, want)
    print("lpips_alex_grad device error: %s %s (bar %.3e)" % (label, " ".join("zero" if e is None else "%.3e" % e for e in errs), bar))
    assert torch.isfinite(got).all()
    for n, e in enumerate(errs):
        if e is None:
            assert float(go[n]) == 0 and torch.all(got[n] == 0), (label, n)
        else:
            assert e <= bar, (label, n, e, bar)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradient_matches_float64_autograd(alex, alex_dead, yardstick, case):
    cases, bars = yardstick
    pred, target, normalize, go, want, want_lpips = cases[case]
    model = alex_dead if case[4] == "dead" else alex
    bar = bars[kind_of_bar(case[4])]
    lpips, got = _grad(model, pred.cuda(), target.cuda(), go, normalize)
    torch.cuda.synchronize()
    rel = ((lpips.cpu().double() - want_lpips).abs() / want_lpips.abs()).max().item()
    print("lpips_alex_grad device value: %s relative error %.3e" % (case_id(case), rel))
    _check(got, want, go, bar, case_id(case))
    # (a sanity check only: the value has its own tests.  Asserted on the dead case too: AlexNet's distance kernel forms the
    #  difference of the unit vectors before it squares it, so an all-zero pixel against a live one costs it nothing)
    assert rel <= 1e-2
    if case[1] == 1 and case[2] == 34:
        assert torch.all(got[:, :, 33] == 0) and got[0, :, 32].abs().max() > 0      # input row 33 is in no conv1 window
    if case == STRIDED:
        # pred as a view with image, channel and row strides of a larger leaf: read in place, the same bits
        n, c, h, w, _ = case
        big = torch.zeros(n + 1, c + 2, h + 7, w + 11, device="cuda")
        big[1:, 1:1 + c, 3:3 + h, 5:5 + w] = pred.cuda()
        view = big.requires_grad_(True)[1:, 1:1 + c, 3:3 + h, 5:5 + w]
        assert not view.is_contiguous() and view.stride(3) == 1
        lpips_v, got_v = _grad(model, view, target.cuda(), go, normalize)
        assert torch.equal(lpips_v, lpips) and torch.equal(got_v, got)


def test_an_identical_pair_has_a_zero_gradient(alex):
    pred, _, _ = make_pair((2, 3, 35, 39, "random"))
    lpips, g = _grad(alex, pred.cuda(), pred.clone().cuda(), torch.tensor([1.5, -0.5]))
    assert torch.all(lpips == 0) and torch.all(g == 0)


@pytest.mark.parametrize("shape", [(1, 3, 31, 31), (2, 1, 34, 38), (3, 3, 71, 93), (2, 3, 64, 80)], ids=lambda s: "%dx%dx%dx%d" % s)
def test_the_forward_value_equals_the_score_bit_for_bit(alex, shape):
    pred, target, _ = make_pair(shape + ("unclamped",))
    pred, target = pred.cuda(), target.cuda()
    for normalize in (True, False):
        want = alex(pred, target, normalize=normalize)
        got = alex.loss(pred.requires_grad_(True), target, normalize=normalize)
        assert got.requires_grad and torch.equal(got.detach(), want) and torch.all(want > 0)
        assert torch.equal(alex.loss(pred.detach(), target, normalize=normalize), want)      # (without a graph: the same value)


def test_two_runs_are_bit_identical(alex):
    pred, target, _ = make_pair((3, 3, 71, 93, "near"))
    go = grad_out_of(3)
    a = _grad(alex, pred.cuda(), target.cuda(), go)
    b = _grad(alex, pred.cuda(), target.cuda(), go)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1][0].abs().max() > 0 and a[1][2].abs().max() > 0


def test_non_finite_values_stay_in_their_pair(alex):
    pred, target, _ = make_pair((3, 3, 35, 43, "random"))
    go = torch.tensor([1.5, 1.0, -0.5])
    clean_lpips, clean = _grad(alex, pred.cuda(), target.cuda(), go)
    for where in ("pred", "target"):
        p, t = pred.clone(), target.clone()
        if where == "pred":
            p[1, 2, 10, 20] = float("nan")
        else:
            t[1, 0, 34, 5] = float("inf")               # the last row: conv1's last window still reads it
        lpips, g = _grad(alex, p.cuda(), t.cuda(), go)
        torch.cuda.synchronize()
        assert torch.isnan(lpips[1]) and torch.isnan(g[1]).all(), where
        assert torch.equal(g[[0, 2]], clean[[0, 2]]) and torch.equal(lpips[[0, 2]], clean_lpips[[0, 2]]), where
    assert torch.isfinite(clean).all() and clean[0].abs().max() > 0 and clean[2].abs().max() > 0


def test_no_torch_convolution_pooling_or_relu_on_the_path(alex, monkeypatch):
    import torch.nn.functional as F
    pred, target, _ = make_pair((2, 3, 40, 40, "random"))
    go = grad_out_of(2)
    want = _grad(alex, pred.cuda(), target.cuda(), go)

    def refuse(*a, **k):
        raise AssertionError("torch convolution / pooling / ReLU called on the LPIPS loss path")

    for name in ("conv2d", "max_pool2d", "relu", "conv_transpose2d"):
        monkeypatch.setattr(F, name, refuse)
    for name in ("conv2d", "max_pool2d", "relu", "conv_transpose2d"):
        monkeypatch.setattr(torch, name, refuse)
    got = _grad(alex, pred.cuda(), target.cuda(), go)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and want[1][0].abs().max() > 0


def test_a_captured_forward_and_backward_replays_on_new_inputs(alex):
    case = (2, 3, 40, 44, "unclamped")
    go = grad_out_of(2).cuda()
    first, second = make_pair(case, seed=1), make_pair(case, seed=2)
    static_p, static_t = first[0].cuda().requires_grad_(True), first[1].cuda()

    def step():
        out = alex.loss(static_p, static_t)
        (g,) = torch.autograd.grad(out, static_p, go)
        return out.detach(), g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                        # (the eager pass every capture here runs first: it leaves the workspace)
    torch.cuda.current_stream().wait_stream(side)
    pool = len(alex._train_pool)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        out, g = step()
    assert len(alex._train_pool) == pool and any(e.captured for e in alex._train_pool)      # nothing was allocated in the capture
    for pred, target, _ in (second, first):
        with torch.no_grad():
            static_p.copy_(pred.cuda())
            static_t.copy_(target.cuda())
        graph.replay()
        torch.cuda.synchronize()
        want = _grad(alex, pred.cuda(), target.cuda(), go)
        assert torch.equal(out, want[0]) and torch.equal(g, want[1]) and want[1][0].abs().max() > 0
    assert not torch.equal(second[0], first[0])


def test_perceptual_loss_differentiates_on_two_channels(weights, yardstick):
    from loss import perceptual_loss
    lin_path, backbone_path, (ws, bs, heads) = weights
    loss = perceptual_loss(weight=2.0, net="alex", lin_path=lin_path, backbone_path=backbone_path, train=True)
    pred, target, _ = make_pair((2, 2, 33, 37, "random"))
    p = pred.cuda().requires_grad_(True)
    v = loss(p, target.cuda())
    assert v.dim() == 0 and v.requires_grad
    v.backward()
    with torch.no_grad():
        assert torch.equal(loss(p, target.cuda()), v.detach())              # the score path: the same value
    # weight * mean over the pairs of the mean over the channels
    each = torch.full((2,), 2.0 / (2 * 2))
    want = torch.cat([ref_grad(pred[:, i:i + 1], target[:, i:i + 1], ws, bs, heads, each)[0] for i in range(2)], 1)
    _check(p.grad, want, each, yardstick[1]["random"], "perceptual_loss 2 channels")
    # every other call returns what it returned: no graph without grad mode or without a pred that requires grad
    assert not loss(pred.cuda(), target.cuda()).requires_grad
    # and without train=True the same object is a score even for a pred that requires grad
    score = perceptual_loss(weight=2.0, net="alex", lin_path=lin_path, backbone_path=backbone_path)
    assert not hasattr(score.model, "loss") and not score(p, target.cuda()).requires_grad


# ------------------------------------------------------------------ the Engine hook
class _Recording:
    """A PerceptualTerm that keeps what it was given and what it returned."""

    def __init__(self, term):
        self.term, self.seen = term, []

    def __call__(self, pred, target):
        value = self.term(pred, target)
        self.seen.append((pred.detach().clone(), target.detach().clone(), value.detach().clone()))
        return value


def _engine(lr=1e-3, **kw):
    from ebfi_amd.engine import Engine
    return Engine(SMALL, device="cuda", precision="bf16x3", lr=lr, seed=7, **kw)


def test_engine_with_the_alex_term_adds_its_value(alex):
    from ebfi_amd.engine import synthetic_batch
    from ebfi_amd.loss import PerceptualTerm
    batch = synthetic_batch(2, 32, 32, device="cuda", seed=11)
    plain = _engine()
    loss_plain = plain.train_step(*batch).clone()
    weight = 0.25
    rec = _Recording(PerceptualTerm(alex, weight))
    with_term = _engine(perceptual=rec)
    loss_with = with_term.train_step(*batch).clone()
    torch.cuda.synchronize()
    (sharp, target, value), = rec.seen
    assert sharp.shape == target.shape == (2, 3, 32, 32) and sharp.dtype == torch.float32
    lpips = alex(sharp, target)
    assert torch.all(lpips > 0) and torch.equal(value, weight * lpips.mean())
    # loss_with - loss_without = w * lpips.mean(): the float32 sum of the two terms, exactly
    assert torch.equal(loss_with, loss_plain + value) and loss_with > loss_plain
    assert not torch.equal(with_term.bucket.flat, plain.bucket.flat)
    assert torch.isfinite(with_term.bucket.flat).all()
    # the LPIPS weights are no parameters of the model and enter no checkpoint
    assert with_term.bucket.numel == plain.bucket.numel
    assert set(with_term.model.state_dict()) == set(plain.model.state_dict())


def test_engine_graph_step_with_the_alex_term_equals_the_eager_one(alex):
    """The bounds and the learning rate (1e-4) of test_engine_graph_step_with_a_term_equals_the_eager_one (test_gpu_lpips_vgg_grad):
    the DCN data gradient sums with atomics, so two runs of a step agree to rounding, not to the bit."""
    from ebfi_amd.engine import synthetic_batch
    from ebfi_amd.loss import PerceptualTerm
    term = PerceptualTerm(alex, 0.25)
    engines = [_engine(lr=1e-4, perceptual=term, graph=g, strict_graph=g) for g in (False, True)]
    for it in range(5):                              # two eager calibration steps, the capture, two replays
        batch = synthetic_batch(2, 32, 32, device="cuda", seed=100 + it)
        losses = [e.train_step(*batch) for e in engines]
        assert torch.allclose(losses[0], losses[1], rtol=1e-5, atol=0), (it, losses)
    torch.cuda.synchronize()
    assert len(engines[1]._graphs) == 1 and not engines[1].graph_capture_failed and engines[1].use_graph
    for (n, a), b in zip(engines[0].model.named_parameters(), engines[1].model.parameters()):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-5), (n, float((a - b).abs().max()))
