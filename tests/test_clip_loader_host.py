"""The prefetching batch generators of ebfi_amd.clipdata (`batches` / `eval_batches` with prefetch >= 1) on a stub dataset that
needs no GPU: which thread runs which half of an item, that order and contents are those of the synchronous path, where a
worker's exception surfaces, and that the worker is gone when the generator is.  Plus the binding of the entry point the device
loader calls (ebfi_period_frames_u8)."""
import threading

import pytest
import torch

from ebfi_amd import _native as N
from ebfi_amd import clipdata

JOIN_TIMEOUT = 30.0      # seconds: every wait in this file is bounded


class Stub:
    """Items are CPU tensors computed from (index, seed); records the thread of every call."""

    def __init__(self, n=7, fail_at=None):
        self.n, self.fail_at = n, fail_at
        self.prepare_threads, self.finish_threads, self.getitem_calls, self.prepared = [], [], [], []

    def __len__(self):
        return self.n

    def prepare(self, index, seed=None):
        self.prepare_threads.append(threading.get_ident())
        if index == self.fail_at:
            raise KeyError("item %d" % index)
        self.prepared.append(index)
        return {"index": index, "seed": seed}

    def finish(self, prepared):
        self.finish_threads.append(threading.get_ident())
        g = torch.Generator().manual_seed(prepared["seed"])
        return {"x": torch.rand(2, 3, generator=g) + prepared["index"], "i": torch.tensor([prepared["index"], prepared["seed"]])}

    def __getitem__(self, index, seed=None):
        self.getitem_calls.append(index)
        return self.finish(self.prepare(index, seed))


def _bounded(fn):
    """Run fn on a thread of its own and wait at most JOIN_TIMEOUT for it: a hang fails the test instead of stalling it."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:
            box["error"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(JOIN_TIMEOUT)
    assert not t.is_alive(), "timed out"
    if "error" in box:
        raise box["error"]
    return box["value"]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y)
        for k in x:
            assert torch.equal(x[k], y[k]), k


def test_prepare_runs_off_the_consuming_thread_and_finish_on_it():
    ds = Stub()
    me = threading.get_ident()
    got = list(clipdata.batches(ds, 2, seed=1, epochs=2, prefetch=1))
    assert len(got) == 6 and len(ds.prepare_threads) == len(ds.finish_threads) == 12
    assert me not in ds.prepare_threads and len(set(ds.prepare_threads)) == 1          # one worker
    assert set(ds.finish_threads) == {me}
    assert ds.getitem_calls == []
    # the synchronous path still goes through __getitem__, on this thread
    ds0 = Stub()
    list(clipdata.batches(ds0, 2, seed=1, epochs=1, prefetch=0))
    assert len(ds0.getitem_calls) == 6 and set(ds0.prepare_threads) == {me}


@pytest.mark.parametrize("prefetch", [1, 2, 5])
def test_order_and_contents_equal_the_synchronous_path(prefetch):
    ref = list(clipdata.batches(Stub(), 2, seed=1, epochs=2, prefetch=0))
    _same(list(clipdata.batches(Stub(), 2, seed=1, epochs=2, prefetch=prefetch)), ref)
    assert not torch.equal(ref[0]["i"], ref[3]["i"])                 # the second epoch is another permutation / other seeds
    _same(list(clipdata.eval_batches(Stub(), 3, seed=4, prefetch=prefetch)), list(clipdata.eval_batches(Stub(), 3, seed=4)))


@pytest.mark.parametrize("prefetch", [1, 2])
def test_sharding_and_drop_last_behave_as_without_prefetch(prefetch):
    for rank in range(3):
        for drop_last in (True, False):
            for shuffle in (True, False):
                kw = dict(rank=rank, world=3, seed=2, epochs=2, shuffle=shuffle, drop_last=drop_last)
                ref = list(clipdata.batches(Stub(11), 2, prefetch=0, **kw))
                mine = len(range(11)[rank::3])                        # 11 items: the ranks get 4, 4 and 3
                assert len(ref) == 2 * (mine // 2 if drop_last else -(-mine // 2))
                _same(list(clipdata.batches(Stub(11), 2, prefetch=prefetch, **kw)), ref)
            kw = dict(rank=rank, world=3, seed=2, drop_last=drop_last)
            ref = list(clipdata.eval_batches(Stub(11), 3, prefetch=0, **kw))
            assert len(ref) == (1 if drop_last else 2)                # 4 items a rank (padded by wrapping): 3 + 1
            _same(list(clipdata.eval_batches(Stub(11), 3, prefetch=prefetch, **kw)), ref)
    ranks = [torch.cat([b["i"][:, 0] for b in clipdata.batches(Stub(12), 2, rank=r, world=3, seed=2, epochs=1, prefetch=1)])
             for r in range(3)]
    assert sorted(torch.cat(ranks).tolist()) == list(range(12))       # the ranks' shards partition the epoch


@pytest.mark.parametrize("prefetch", [1, 3])
def test_a_failing_prepare_surfaces_at_its_own_batch(prefetch):
    """Items in file order, batches of 2: item 5 sits in the third batch.  The first two batches arrive whole, the third raises
    the worker's exception -- even when the worker met it while the consumer was still at the first batch."""
    ds = Stub(8, fail_at=5)
    it = clipdata.batches(ds, 2, seed=0, epochs=1, shuffle=False, prefetch=prefetch)
    first, second = _bounded(lambda: next(it)), _bounded(lambda: next(it))
    assert first["i"][:, 0].tolist() == [0, 1] and second["i"][:, 0].tolist() == [2, 3]
    with pytest.raises(KeyError, match="item 5"):
        _bounded(lambda: next(it))
    with pytest.raises(StopIteration):
        _bounded(lambda: next(it))
    assert ds.prepared == [0, 1, 2, 3, 4]                              # nothing past the failure was started


def test_the_worker_runs_at_most_prefetch_batches_ahead():
    ds = Stub(20)
    it = clipdata.batches(ds, 2, seed=0, epochs=1, shuffle=False, prefetch=2)
    _bounded(lambda: next(it))
    # the consumer holds batch 0; the worker may have made batches 1 and 2 and nothing of batch 3
    assert max(ds.prepared) <= 5
    _bounded(it.close)


def test_close_and_exhaustion_join_the_worker():
    before = threading.active_count()
    it = clipdata.batches(Stub(), 2, seed=1, prefetch=1)                # endless
    _bounded(lambda: [next(it) for _ in range(5)])
    assert threading.active_count() == before + 1
    _bounded(it.close)
    assert threading.active_count() == before
    _bounded(lambda: list(clipdata.batches(Stub(), 2, seed=1, epochs=1, prefetch=2)))
    assert threading.active_count() == before
    _bounded(lambda: list(clipdata.eval_batches(Stub(), 2, prefetch=1)))
    assert threading.active_count() == before
    it = clipdata.batches(Stub(8, fail_at=1), 2, seed=0, epochs=1, shuffle=False, prefetch=1)
    with pytest.raises(KeyError):
        _bounded(lambda: next(it))
    assert threading.active_count() == before
    # a generator that is made and never started owns no thread
    clipdata.batches(Stub(), 2, prefetch=1)
    assert threading.active_count() == before


def test_dataset_halves_compose_and_the_frames_keyword_is_checked(tmp_path):
    path = clipdata.write_synthetic_clip(str(tmp_path / "c.npz"), num_imgs=9, H=12, W=20, events_per_frame=20, seed=1)
    with pytest.raises(ValueError, match="frames"):
        clipdata.ClipDataset(path, frames_per_period=4, frames_per_blurry=2, device="cpu", frames="gpu")
    ds = clipdata.ClipDataset(path, time_bins=2, frames_per_period=4, frames_per_blurry=3, crop=[8, 12], center_crop=[4, 8],
                              flips=True, noise=(1.0, 0.5), device="cpu", frames="device")
    assert clipdata.ClipDataset(path, frames_per_period=4, frames_per_blurry=2, device="cpu").frames == "host"
    for seed in (5, 1, 0, 3):
        i, j, h, w = ds.window((12, 20), seed)
        t = torch.arange(12 * 20.0).reshape(1, 12, 20)
        fh, fv = ds.flip_decisions(seed)
        ref = t[..., i:i + h, j:j + w]
        ref = ref.flip(-1) if fh else ref
        ref = ref.flip(-2) if fv else ref
        assert (h, w) == (4, 8) and torch.equal(ds.augment([t], (12, 20), seed)[0], ref)       # one window == augment's crops
        p = ds.prepare(1, seed)
        assert not p["stage"].is_pinned() and p["stage"].shape == (4, 4, 20, 3) and p["num_blur"] == 3
        assert torch.equal(p["stage"], torch.from_numpy(ds.clips[0].images[4:8, i:i + h]))      # the window's rows, as stored
        assert p["noise"].shape == (1, 2, 2, 4, 8) and p["noise"].dtype == torch.int32
    assert [ds.flip_decisions(s) for s in (5, 1, 0, 3)] == [(False, False), (True, False), (False, True), (True, True)]


def test_period_frames_entry_point_is_declared_and_bound():
    assert "ebfi_period_frames_u8" in N.declared_symbols() and "ebfi_period_frames_u8" in N.SIGNATURES
    header = open(N.HEADER).read()
    assert "#define EBFI_ABI_VERSION 14" in header and N.ABI_VERSION == 14          # a pure addition: the generation stays
    lib = N.lib()
    assert lib.ebfi_abi_version() == 14
    import ctypes
    s3 = (ctypes.c_int64 * 3)(48, 12, 3)
    p = ctypes.c_void_p(16)
    # argument errors are refused before anything touches the GPU (none is needed here)
    assert lib.ebfi_period_frames_u8(p, s3, 2, 0, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, p, None) == -1 and b"n_blur" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(p, s3, 2, 3, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, p, None) == -1 and b"n_blur" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(p, s3, 0, 0, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, p, None) == -1
    assert lib.ebfi_period_frames_u8(p, s3, 2, 1, 4, 4, 0, 0, 4, 4, 0, 0, 0, None, p, None) == -1 and b"null" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(p, s3, 2, 1, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, None, None) == -1 and b"null" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(None, s3, 2, 1, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, p, None) == -1 and b"null" in lib.ebfi_last_error()
    for win in ((0, 0, 5, 4), (1, 0, 4, 4), (0, 2, 4, 3), (-1, 0, 2, 2), (0, 0, 0, 4)):
        assert lib.ebfi_period_frames_u8(p, s3, 2, 1, 4, 4, *win, 0, 0, 0, p, p, None) == -1 and b"window" in lib.ebfi_last_error()
    assert lib.ebfi_period_frames_u8(p, (ctypes.c_int64 * 3)(48, 12, 2), 2, 1, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, p, None) == -1
    assert lib.ebfi_period_frames_u8(p, (ctypes.c_int64 * 3)(-48, 12, 3), 2, 1, 4, 4, 0, 0, 4, 4, 0, 0, 0, p, p, None) == -1
    with pytest.raises(NotImplementedError):
        from ebfi_amd import frameio
        frameio.period_to_planar(torch.zeros(2, 4, 4, 3, dtype=torch.uint8), 1)
