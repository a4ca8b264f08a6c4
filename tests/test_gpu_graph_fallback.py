"""The branch a refused hipGraph capture takes, for its three callers (Engine, ExposureEngine, ClipInterpolator): eager launches
with the same results, or a RuntimeError under strict_graph.  No capture is attempted and nothing is provoked on the device:
ebfi_amd.graphstep.capture is replaced by a function that raises what torch raises when a capture cannot be taken."""
import pytest
import torch

from test_gpu_validation import SMALL

pytestmark = pytest.mark.gpu

REFUSAL = "capture refused\nsecond line"


def _refuse(monkeypatch):
    from ebfi_amd import graphstep
    calls = []

    def refused(fn, device, warmups, before=None):
        calls.append(warmups)
        raise RuntimeError(REFUSAL)

    monkeypatch.setattr(graphstep, "capture", refused)
    return calls


def _stage2(**kw):
    from ebfi_amd.engine import Engine, synthetic_batch
    return Engine(SMALL, device="cuda", precision="bf16x3", lr=1e-3, seed=7, **kw), synthetic_batch(2, 32, 32, device="cuda", seed=11)


def _stage1(**kw):
    from ebfi_amd.exposure_engine import ExposureEngine, synthetic_exposure_batch
    return (ExposureEngine(device="cuda", precision="bf16x3", lr=1e-3, seed=7, **kw),
            synthetic_exposure_batch(2, 32, 32, device="cuda", seed=11))


@pytest.mark.parametrize("make,prefix", [(_stage2, "ebfi_amd.engine:"), (_stage1, "ebfi_amd.exposure_engine:")], ids=["Engine", "ExposureEngine"])
def test_refused_capture_continues_eagerly_or_raises_under_strict_graph(make, prefix, monkeypatch, capfd):
    twin, batch = make(graph=False)
    want = [twin.train_step(*batch).clone() for _ in range(3)]
    calls = _refuse(monkeypatch)
    eng, _ = make(graph=True, strict_graph=False)
    assert eng.use_graph and not eng.graph_capture_failed
    got = [eng.train_step(*batch).clone() for _ in range(3)]
    torch.cuda.synchronize()
    assert calls == [2]                                            # one attempt (two warm-up passes asked for), never a second
    assert eng.graph_capture_failed and eng.graph_capture_error == "capture refused" and not eng.use_graph and not eng._graphs
    err = capfd.readouterr().err
    assert err.count("hipGraph capture failed") == 1
    assert prefix + " hipGraph capture failed (capture refused); continuing with eager launches" in err and "second line" not in err
    assert eng.iteration == twin.iteration == 3
    assert all(torch.equal(a, b) for a, b in zip(got, want)), (got, want)
    assert torch.equal(eng.optimizer.flat.detach(), twin.optimizer.flat.detach())
    strict, _ = make(graph=True, strict_graph=True)
    with pytest.raises(RuntimeError, match="strict_graph") as info:
        for _ in range(3):                                         # (Engine captures after its two calibration steps)
            strict.train_step(*batch)
    assert str(info.value).startswith(prefix) and "capture refused" in str(info.value) and "second line" not in str(info.value)
    assert strict.use_graph and not strict.graph_capture_failed


def test_engine_guard_words_are_restored_after_a_refused_capture(monkeypatch):
    """The guard words are saved ahead of the warm-up passes and put back when the capture fails.  It matters when the capture
    falls into the middle of an accumulation window, where nothing clears the guard any more: a flag left behind by the failed
    attempt would skip the window's optimiser step.  The stand-in leaves such a flag (and a skipped-step count) behind."""
    from ebfi_amd import graphstep
    eng, batch = _stage2(graph=False, accu_step=2)
    for _ in range(2 * eng.calibration_steps + 1):
        eng.train_step(*batch)
    assert eng._micro == 1 and not eng._calibrating()
    eng.use_graph = True                                       # the next call wants a graph: mid-window
    guard = eng._guard()
    before, steps = guard.clone(), eng.iteration

    def refused(fn, device, warmups, before=None):
        guard.copy_(torch.tensor([1, 9], dtype=torch.int32, device="cuda"))
        raise RuntimeError(REFUSAL)

    monkeypatch.setattr(graphstep, "capture", refused)
    eng.train_step(*batch)
    torch.cuda.synchronize()
    assert eng.graph_capture_failed and not eng.use_graph
    assert torch.equal(guard, before), (guard, before)
    assert eng.iteration == steps + 1 and eng.book.skipped_steps() == 0


def test_interpolator_continues_eagerly_after_a_refused_capture(monkeypatch, capfd):
    from ebfi_amd.engine import DEFAULT_MODEL_ARGS, ClipInterpolator, synthetic_batch
    from ebfi_amd.model import EVFIAutoEx
    torch.manual_seed(7)
    model = EVFIAutoEx(**dict(DEFAULT_MODEL_ARGS, **SMALL)).cuda()
    frame, event, _, gtex, _ = synthetic_batch(2, 32, 32, device="cuda", seed=12)
    stamps = [0.25, 0.5, 0.75]
    want = ClipInterpolator(model, precision="bf16x3", graph=False)(frame, event, gtex, stamps)
    calls = _refuse(monkeypatch)
    interp = ClipInterpolator(model, precision="bf16x3", graph=True)
    got = interp(frame, event, gtex, stamps)
    again = interp(frame, event, gtex, stamps)
    assert calls == [1] and interp.graph_capture_failed and interp.graph_capture_error == "capture refused"
    assert not interp.graph and not interp._captured
    assert torch.equal(got, want) and torch.equal(again, want)
    err = capfd.readouterr().err
    assert err.count("ebfi_amd.engine: hipGraph capture of the inference step failed (capture refused); continuing with eager launches") == 1
