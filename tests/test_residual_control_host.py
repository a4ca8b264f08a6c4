"""What tests/test_gpu_residual_control.py relies on, checked on the CPU alone: its float64 restatement of ResidualControl against
oracle/model_ref.residual_control (fp32) and against the module's own CPU forward in double (output and every gradient), the kink
condition for every recorded Tier-A seed, and the case table: shapes, batch predicates and which cases the fused node takes."""
import pytest
import torch

import test_gpu_residual_control as rcg
from oracle import model_ref

# float64 against float64, sums of at most 128 * 9 products over 3 * step layers: measured 0 .. 1e-15
TOL64 = 1e-12
# the oracle computes in fp32: 2^-24 per rounding, ~sqrt(1152) roundings per sum, 3 * step + 1 <= 7 layers deep -> ~6e-6 at worst
TOL32 = 1e-5

CASE_SLOPES = [(c, s) for c in rcg.CASES for s in rcg.SLOPES[c.tier]]
IDS = ["%s-slope%g" % (c.id, s) for c, s in CASE_SLOPES]


def _rel(got, ref):
    return ((got.detach().double() - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(case, slope):
        if (case.id, slope) not in cache:
            cache[(case.id, slope)] = rcg.build_reference(case, slope)
        return cache[(case.id, slope)]
    return get


@pytest.mark.parametrize("case,slope", CASE_SLOPES, ids=IDS)
def test_restatement_is_the_module_in_double(case, slope, refs):
    """Output, input gradients and every parameter gradient of the restatement equal those of ResidualControl.forward on CPU
    tensors (torch's own convolutions, layer by layer) in float64."""
    ref = refs(case, slope)
    rc = rcg.make_module(case, slope).double()
    rc.load_state_dict({k: v.detach() for k, v in ref.sd.items()})
    data, ex, t = (v.detach().clone().requires_grad_() for v in (ref.data, ref.ex, ref.t))
    out = rc(data, ex, t)
    out.backward(ref.g)
    assert out.shape == ref.out.shape and _rel(out, ref.out) < TOL64
    assert torch.isfinite(ref.out).all() and ref.out.abs().max() > 1e-2
    assert _rel(data.grad, ref.data.grad) < TOL64 and _rel(ex.grad, ref.ex.grad) < TOL64 and _rel(t.grad, ref.t.grad) < TOL64
    named = dict(rc.named_parameters())
    assert set(named) == set(ref.sd) and len(named) == 14 * case.step
    for n, q in ref.sd.items():
        assert q.grad.abs().max() > 0 and _rel(named[n].grad, q.grad) < TOL64, n


@pytest.mark.parametrize("case", rcg.CASES, ids=[c.id for c in rcg.CASES])
def test_restatement_against_the_fp32_oracle(case, refs):
    """The oracle states the default activation (slope 0.01) only."""
    ref = refs(case, 0.01)
    sd = {"ResidualControl." + k: v.detach().float() for k, v in ref.sd.items()}
    with torch.no_grad():
        got = model_ref.residual_control(sd, "ResidualControl", ref.data.detach().float(), ref.ex.detach().float(),
                                         ref.t.detach().float(), case.step)
    assert got.dtype == torch.float32 and _rel(got, ref.out) < TOL32


@pytest.mark.parametrize("case", [c for c in rcg.CASES if c.tier == "A"], ids=[c.id for c in rcg.CASES if c.tier == "A"])
def test_recorded_seed_keeps_every_activation_off_its_kink(case, refs):
    """With the recorded seed every LeakyReLU pre-activation of the float64 reference -- seven layers per round, the scalar layers
    Conv1 / Conv2 included -- has |z| >= KINK * max|z|: no device rounding can pick another subgradient."""
    ref = refs(case, 0.01)
    assert 0 <= case.seed <= 255
    assert ref.n_act == 7 * case.step
    assert ref.kink >= rcg.KINK, (case.id, case.seed, ref.kink)


def test_tier_b_is_the_identity_activation(refs):
    """Slope 1.0: the restatement is linear in the upstream gradient's path -- the derivative of every activation is 1."""
    case = rcg.BY_ID["b-128-s1-b1-13x36"]
    assert rcg.SLOPES["B"][0] == 1.0
    rc = rcg.make_module(case, 1.0)
    slopes = {m.negative_slope for m in rc.modules() if isinstance(m, torch.nn.LeakyReLU)}
    assert slopes == {1.0}
    z = torch.randn(64, dtype=torch.float64)
    assert torch.equal(torch.nn.functional.leaky_relu(z, 1.0), z)


def test_case_table():
    """The shapes the issue names, the batch predicate of each, and which route the shape alone decides."""
    assert len({c.id for c in rcg.CASES}) == len(rcg.CASES)
    shape = lambda c: (c.C, c.step, c.B, c.H, c.W)
    a = {shape(c) for c in rcg.CASES if c.tier == "A"}
    assert a == {(64, 1, 1, 1, 4), (64, 2, 1, 2, 4), (64, 2, 2, 2, 4), (128, 1, 1, 2, 4), (64, 2, 1, 2, 6), (64, 1, 2, 4, 4),
                 (64, 1, 1, 3, 3), (32, 1, 1, 2, 4)}
    want_b = {(64, 2, 2, 40, 64): True, (64, 2, 2, 36, 64): False, (64, 1, 1, 37, 100): True, (128, 1, 1, 13, 36): False,
              (64, 1, 2, 10, 34): False}
    b = {shape(c): rcg.batched(c.C, c.B, c.H, c.W) for c in rcg.CASES if c.tier == "B"}
    assert b == want_b
    assert not any(rcg.batched(c.C, c.B, c.H, c.W) for c in rcg.CASES if c.tier == "A")
    tiles = lambda c: c.B * -(-c.H // 4) * -(-c.W // 32)
    assert tiles(rcg.BY_ID["b-64-s2-b2-40x64"]) == 40 and tiles(rcg.BY_ID["b-64-s2-b2-36x64"]) == 36 and \
        tiles(rcg.BY_ID["b-64-s1-b1-37x100"]) == 40
    # the largest float64 reference
    assert max(c.B * c.C * c.H * c.W * c.step for c in rcg.CASES) == 2 * 64 * 40 * 64 * 2
    # the node refuses exactly the two fallback cases; rows without quads take no images
    assert [c.id for c in rcg.CASES if not rcg.node_usable(c)] == ["a-64-s1-b1-3x3-fallback", "a-32-s1-b1-2x4-fallback"]
    assert [c.id for c in rcg.CASES if rcg.node_usable(c) and c.W % 4 != 0] == ["a-64-s2-b1-2x6", "b-64-s1-b2-10x34"]
    for c in rcg.CASES:
        assert set(c.modes) <= set(rcg.ALL_MODES)
        assert ("book" in c.modes) == rcg.node_usable(c)


def test_module_predicates_agree_with_the_table():
    """rc_fused.fusable holds for every module the cases build (one slope on all layers), so `usable` is decided by the shape."""
    from ebfi_amd import rc_fused
    for case, slope in CASE_SLOPES:
        assert rc_fused.fusable(rcg.make_module(case, slope)), case.id


def test_expected_routes_are_complete():
    """Every pass of every mode has a stated route; the image passes differ from pass 1 and from each other where they should."""
    for c in rcg.CASES:
        for m in c.modes:
            whats = {"nograd": ["nograd"], "book": list(rcg.BOOK_PASSES), "book-all": ["all-1", "all-2"]}.get(m, ["train"])
            routes = [rcg.expected_route(c, m, w) for w in whats]
            assert all(r and all(n > 0 for n in r.values()) for r in routes), (c.id, m)
            if m == "book" and c.W % 4 == 0:
                one, two, three, restored, after = routes
                assert two == three == after and one != two and restored != two and restored != one
                assert ("conv_wgrad_f16_tr/img_batch" in two) == rcg.batched(c.C, c.B, c.H, c.W)
            elif m == "book":
                assert all(r == routes[0] for r in routes)
