"""Host-side checks of the STGAN adversarial loss (ebfi_amd.gan, tests/stgan_ref.py): the float64 restatement against the
reference's own numbers, the module interface, every refusal, the neighbour law of the clip reader and the Adamax state layout.
Nothing here computes on a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stgan_ref as R  # noqa: E402

from ebfi_amd import _native as N  # noqa: E402
from ebfi_amd import clipdata  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.2


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(HERE, "golden", "stgan_small.npz"))


@pytest.fixture(scope="module")
def built_lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) <= rel * float(np.abs(want).max())


def test_restatement_agrees_with_the_reference_in_float64(fixture):
    """tests/golden/stgan_small.npz was written by the reference's own loss/adversarial.py (tests/golden/make_stgan_golden.py):
    P = 32, B = 3, two consecutive calls.  The restatement is a different program for the same law: 1e-12 of each output's scale."""
    names = [n for n, _ in R.names_and_shapes(32)]
    assert [str(n) for n in fixture["names"]] == names
    assert [str(s) for s in fixture["shapes"]] == [str(tuple(s)) for _, s in R.names_and_shapes(32)]
    ref = R.RefAdversarial(32, R.fill_state(20, 32))
    pn = ref.param_names
    assert len(pn) == 52 and sum(ref.state[n].numel() for n in pn) == 674249
    for c in range(2):
        loss_d, loss_g, grad = ref.call(*(R.inputs_from_bytes(fixture[k][c]) for k in ("fake_u8", "real_u8", "frames_u8")))
        assert _close(loss_d, fixture["loss_d"][c]) and _close(loss_g, fixture["loss_g"][c])
        assert _close(grad.numpy(), fixture["grad_fake"][c])
        run = np.concatenate([ref.state[n].numpy() for n in names if n.endswith("running_mean")] +
                             [ref.state[n].numpy() for n in names if n.endswith("running_var")])
        assert _close(run, fixture["running"][c])
        assert [int(ref.state[n]) for n in names if n.endswith("num_batches_tracked")] == fixture["tracked"][c].tolist()
        assert _close([float(ref.state[n].sum()) for n in pn], fixture["param_sums"][c])
        heads = np.zeros((52, 8))
        for i, n in enumerate(pn):
            h = ref.state[n].reshape(-1)[:8].numpy()
            heads[i, :len(h)] = h
        assert _close(heads, fixture["param_heads"][c])
    assert os.path.getsize(os.path.join(HERE, "golden", "stgan_small.npz")) < 300 * 1024


def test_module_interface_is_the_references(fixture):
    from ebfi_amd import gan
    from loss import Adversarial, ST_Discriminator
    from loss.adversarial import Adversarial as A2
    from loss.discriminator import ST_Discriminator as D2
    assert Adversarial is gan.Adversarial is A2 and ST_Discriminator is gan.ST_Discriminator is D2
    adv = Adversarial(32, "STGAN")
    sd = adv.state_dict()
    assert len(sd) == 100 and list(sd) == [str(n) for n in fixture["names"]]
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in fixture["shapes"]]
    assert "discriminator.s_features.0.0.weight" in sd and "discriminator.t_features.7.1.num_batches_tracked" in sd
    assert adv.gan_k == 1 and adv.gan_type == "STGAN" and adv.discriminator.views_intact()
    assert sum(p.numel() for p in Adversarial(16).parameters()) == 281033 and sum(p.numel() for p in adv.parameters()) == 674249
    # load_state_dict keeps the flat storage; the restatement's state has the module's names
    adv.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in R.fill_state(1, 32).items()})
    assert adv.discriminator.views_intact()
    assert torch.equal(adv.discriminator.flat[:216].view(8, 3, 3, 3), sd["discriminator.s_features.0.0.weight"])
    # optimiser and scheduler as the reference builds them
    grp = adv.optimizer.param_groups[0]
    assert isinstance(adv.optimizer.inner, torch.optim.Adamax)
    assert (grp["lr"], tuple(grp["betas"]), grp["eps"], grp["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 0)
    s = adv.scheduler
    assert isinstance(s, torch.optim.lr_scheduler.ReduceLROnPlateau)
    assert (s.mode, s.factor, s.patience, s.threshold, s.threshold_mode) == ("max", 0.5, 5, 0.01, "abs")
    for _ in range(7):                      # a plateau: the seventh step halves the lr, and the next launch takes it by value
        s.step(30.0)
    assert adv.lr == 5e-4 == adv.optimizer.param_groups[0]["lr"]
    assert adv.loss_d.dim() == 0 and adv.loss == 0.0 and "loss_d" not in sd


def test_refusals():
    from ebfi_amd.gan import Adversarial, AdversarialTerm, ST_Discriminator
    for other in ("GAN", "WGAN", "WGAN_GP", "T_WGAN_GP", "FI_GAN", "FI_Cond_GAN"):
        with pytest.raises(NotImplementedError, match="STGAN"):
            Adversarial(32, other)
    for P in (24, 40, 8, 0):
        with pytest.raises(ValueError, match="multiple of 16"):
            ST_Discriminator(P)
    adv = Adversarial(16)
    img = lambda *s: torch.rand(*s)
    with pytest.raises(ValueError, match="PatchSize"):                 # H != P
        adv(img(2, 3, 32, 16), img(2, 3, 32, 16), img(2, 2, 3, 32, 16))
    with pytest.raises(ValueError, match="PatchSize"):                 # W != P
        adv(img(2, 3, 16, 32), img(2, 3, 16, 32), img(2, 2, 3, 16, 32))
    with pytest.raises(ValueError, match="more than 1 value"):         # P = 16 at B = 1: one value per channel at the last stage
        adv(img(1, 3, 16, 16), img(1, 3, 16, 16), img(1, 2, 3, 16, 16))
    with pytest.raises(ValueError, match="input_frames"):
        adv(img(2, 3, 16, 16), img(2, 3, 16, 16), None)
    with pytest.raises(NotImplementedError):                           # well-formed CPU tensors: there is no CPU path
        adv(img(2, 3, 16, 16), img(2, 3, 16, 16), img(2, 2, 3, 16, 16))
    for w in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="positive"):
            AdversarialTerm(adv, w)
    assert AdversarialTerm(adv, 0.5).weight == 0.5
    with pytest.raises(RuntimeError, match="evaluation mode"):
        adv.discriminator.eval()
    with pytest.raises(RuntimeError, match="evaluation mode"):
        adv.eval()
    assert adv.discriminator.training and adv.discriminator.train() is adv.discriminator


def test_entry_points_refuse_bad_arguments_without_touching_the_gpu(built_lib):
    lib = built_lib
    p = ctypes.c_void_p(4096)
    assert lib.ebfi_bn_lrelu_forward(p, p, p, p, p, None, None, None, 1, 4, 1, EPS, MOMENTUM, SLOPE, p, 1 << 20, None) == -1     # n == 1
    assert b"more than 1 value" in lib.ebfi_last_error()
    assert lib.ebfi_bn_lrelu_forward(p, p, p, p, p, None, None, None, 2, 4, 4, EPS, MOMENTUM, SLOPE, p, 8, None) == -4            # short workspace
    assert lib.ebfi_bn_lrelu_forward(None, p, p, p, p, None, None, None, 2, 4, 4, EPS, MOMENTUM, SLOPE, p, 1 << 20, None) == -1
    assert lib.ebfi_bn_lrelu_backward(p, p, p, p, p, None, None, None, 2, 4, 4, SLOPE, p, 1 << 20, None) == -1                     # no grad_x
    assert lib.ebfi_adamax_step(p, p, None, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert lib.ebfi_adamax_step(p, ctypes.c_void_p(4100), None, p, p, p, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == -1               # alignment
    assert lib.ebfi_bce_logits_pair(None, None, 4, p, None, None, None) == -1
    assert lib.ebfi_stgan_temporal_forward(p, 2, p, 12, p, 12, p, 2, 12, None) == -1                                               # stride < C*H*W



def test_neighbour_law_through_the_host_loader(tmp_path):
    """dataset.NeedNeighborGT.  The law is from READING the reference's code (dataloader/h5dataset.py:138-147 for the indices,
    :219-271 for the read and the shared augmentation seed): h5py is not installed where this project is built and tested, so no
    fixture could be made by the reference's H5Dataset.  Neighbour 0 of latent i is latent max(i - 1, 0), neighbour 1 is latent
    min(i + 1, NumF - 1), of the same period; the reference reads those frames again and augments them with the item's seed.
    Checked here on write_synthetic_clip data through the host loader against frames read from the clip independently."""
    from oracle import events_ref
    path = clipdata.write_synthetic_clip(str(tmp_path / "c.npz"), num_imgs=13, H=20, W=24, events_per_frame=30, seed=4)
    kw = dict(time_bins=2, frames_per_period=4, frames_per_blurry=2, crop=[16, 16], flips=True, device="cpu")
    assert clipdata.neighbour_indices(4).tolist() == [[0, 1], [0, 2], [1, 3], [2, 3]]
    assert clipdata.neighbour_indices(1).tolist() == [[0, 0]]
    images = np.load(path)["images"]

    def item(ds, i, seed):
        sharp, blur, (xs, ys, ts, ps), duty = ds.host_item(i)
        stack = torch.from_numpy(events_ref.events_to_stack(xs, ys, ts, ps.astype(np.float32), 2, (20, 24))).transpose(0, 1)
        return ds.assemble(*ds.augment([sharp, blur, stack], (20, 24), seed=seed), duty)

    ds = clipdata.ClipDataset(path, neighbours=True, **kw)
    plain = clipdata.ClipDataset(path, **kw)
    assert len(ds) == 3
    samples = []
    for i, seed in ((0, 1), (2, 0)):                                   # (seeds with a horizontal and a vertical flip)
        it = item(ds, i, seed)
        samples.append(it)
        nb = it["SeqNeighborF"]
        assert nb.shape == (1, 1, 4, 2, 3, 16, 16) and nb.dtype == torch.float32
        assert set(it) == set(item(plain, i, seed)) | {"SeqNeighborF"}
        for f in range(4):
            for k, src in enumerate((max(f - 1, 0), min(f + 1, 3))):
                raw = torch.from_numpy(np.ascontiguousarray(images[4 * i + src][:, :, ::-1])).permute(2, 0, 1).float() / 255
                want, = ds.augment([raw], (20, 24), seed=seed)
                assert torch.equal(nb[0, 0, f, k], want), (i, f, k)
        assert torch.equal(nb[0, 0, :, 0, :], it["SeqLatentF"][0, 0, [0, 0, 1, 2]])
    assert any(ds.flip_decisions(s)[0] for s in (1, 0)) and any(ds.flip_decisions(s)[1] for s in (1, 0))
    # model_inputs: six items with the key, the five it has always yielded without
    batch = clipdata.collate(samples)
    assert batch["SeqNeighborF"].shape == (2, 1, 1, 4, 2, 3, 16, 16)
    six = list(clipdata.model_inputs(batch))
    assert len(six) == 4 and all(len(t) == 6 for t in six)
    for f, t in enumerate(six):
        assert t[5].shape == (2, 2, 3, 16, 16) and t[5].is_contiguous() and torch.equal(t[5], batch["SeqNeighborF"][:, 0, 0, f])
        assert torch.equal(t[4], batch["SeqLatentF"][:, 0, 0, f])
    five = list(clipdata.model_inputs(clipdata.collate([item(plain, 0, 1), item(plain, 2, 0)])))
    assert len(five) == 4 and all(len(t) == 5 for t in five)
    assert all(torch.equal(a, b) for s, t in zip(six, five) for a, b in zip(s[:5], t))


def test_dataset_section_turns_the_neighbours_on_or_refuses():
    base = {"scale": 1, "ori_scale": "ori"}
    assert "neighbours" not in clipdata.dataset_args_from_config(base)
    assert "neighbours" not in clipdata.dataset_args_from_config(dict(base, NeedNeighborGT=False))
    assert clipdata.dataset_args_from_config(dict(base, NeedNeighborGT=True))["neighbours"] is True
    with pytest.raises(NotImplementedError, match="DeblurPretrain"):
        clipdata.dataset_args_from_config(dict(base, NeedNeighborGT=True, DeblurPretrain=True))
    assert "neighbours" not in clipdata.dataset_args_from_config(dict(base, DeblurPretrain=True))


def test_adamax_state_dict_interchanges_with_torch():
    """FlatAdamax speaks torch.optim.Adamax's per-parameter layout in both directions (CPU tensors take torch's own step)."""
    from ebfi_amd.gan import Adversarial
    torch.manual_seed(0)
    adv = Adversarial(16)
    D, opt = adv.discriminator, adv.optimizer
    twin_params = [torch.nn.Parameter(p.detach().clone()) for p in D.parameters()]
    twin = torch.optim.Adamax(twin_params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
    g = torch.Generator().manual_seed(1)
    assert opt.state_dict()["state"] == {}
    for _ in range(2):
        grad = torch.randn(D.flat.numel(), generator=g)
        opt.step(grad * 0.25, grad * 0.75)                         # (two buffers: their sum is the gradient)
        for p, v in zip(twin_params, D.grad_views(grad)):
            p.grad = v.clone()
        twin.step()
    assert all(torch.equal(a, b) for a, b in zip(D.parameters(), twin_params)) and D.views_intact()
    sd, want = opt.state_dict(), twin.state_dict()
    assert set(sd["state"]) == set(want["state"]) == set(range(52)) and sd["param_groups"][0]["params"] == list(range(52))
    for i in range(52):
        assert set(sd["state"][i]) == {"step", "exp_avg", "exp_inf"} and float(sd["state"][i]["step"]) == 2
        assert all(torch.equal(sd["state"][i][k], want["state"][i][k]) for k in ("exp_avg", "exp_inf"))
    # torch loads ours ...
    probe_params = [torch.nn.Parameter(p.detach().clone()) for p in D.parameters()]
    probe = torch.optim.Adamax(probe_params, lr=1e-3)
    probe.load_state_dict(sd)
    # ... and ours loads torch's: after one more step on the same gradient all three agree
    torch.manual_seed(5)
    other = Adversarial(16)
    other.discriminator.load_state_dict(D.state_dict())
    want["param_groups"][0]["lr"] = 2.5e-4
    other.optimizer.load_state_dict(want)
    assert other.lr == 2.5e-4
    other.optimizer.param_groups[0]["lr"] = 1e-3
    grad = torch.randn(D.flat.numel(), generator=g)
    opt.step(grad)
    other.optimizer.step(grad)
    for p, v in zip(probe_params, D.grad_views(grad)):
        p.grad = v.clone()
    probe.step()
    assert torch.equal(D.flat, other.discriminator.flat)
    assert all(torch.equal(a, b) for a, b in zip(D.parameters(), probe_params))
    assert float(other.optimizer.state_dict()["state"][51]["step"]) == 3
    with pytest.raises(ValueError, match="parameters"):
        Adversarial(32).optimizer.load_state_dict({"state": {}, "param_groups": [{"params": [0, 1]}]})


def test_trainer_settings_and_checkpoint_keys():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "ebfi-be_amd"))
    import argparse
    import train_ours as T
    assert T.CHECKPOINT_KEYS == ("model", "lr_scheduler", "optimizer", "config", "trainer")
    ns = lambda w=None: argparse.Namespace(gan_weight=w)
    cfg = lambda **tr: {"trainer": dict({"height": 64, "width": 64}, **tr)}
    assert T.adversarial_settings(cfg(), ns()) == (0.0, "STGAN")
    assert T.adversarial_settings(cfg(gan={"weight": 0.01, "type": "STGAN"}), ns()) == (0.01, "STGAN")
    assert T.adversarial_settings(cfg(gan={"weight": 0.01}), ns(0.5)) == (0.5, "STGAN")
    for bad, flag in ((cfg(gan={"weight": 0.1, "type": "WGAN_GP"}), None), (cfg(gan={"weight": -1}), None), (cfg(), -0.5),
                      (cfg(height=64, width=96), 0.1), (cfg(height=40, width=40), 0.1)):
        with pytest.raises(SystemExit):
            T.adversarial_settings(bad, ns(flag))
    assert T.adversarial_settings(cfg(height=40, width=40, gan={"type": "WGAN"}), ns()) == (0.0, "WGAN")     # off: nothing to refuse
    assert T.get_args(["--gan_weight", "0.02"]).gan_weight == 0.02 and T.get_args([]).gan_weight is None
    batch = tuple(torch.zeros(2, 3, 8, 8) for _ in range(5))
    six = T.with_neighbours(batch, 7, on_device=False)
    assert len(six) == 6 and six[5].shape == (2, 2, 3, 8, 8) and torch.equal(six[5], T.with_neighbours(batch, 7, False)[5])
    assert not torch.equal(six[5], T.with_neighbours(batch, 8, False)[5]) and 0 <= float(six[5].min()) and float(six[5].max()) < 1


def test_engine_without_the_term_is_what_it_was():
    """Engine(adversarial=None): no discriminator, the five-input pass, and the stepper's capture hooks are no-ops."""
    from ebfi_amd.engine import Engine
    from ebfi_amd.graphstep import GraphStepper
    small = dict(FrameBasech=8, EventBasech=8, InterCH=8, TB=4, step=2, channels=[4, 4, 8, 8])
    eng = Engine(small, device="cpu", lr=1e-3, seed=1)
    assert eng.adversarial is None and eng.adversarial_term is None and eng._capture_snapshot() is None
    assert eng._graph_key() == (True,) and GraphStepper._capture_snapshot(eng) is None
