"""Host-side checks of the event-count images (ebfi_amd.eventvis, csrc/eventvis.hip, myutils.vis_events): the numpy
restatement the GPU tests use as their oracle reproduces the REFERENCE'S OWN outputs (tests/golden/eventvis_small.npz, written
by tests/golden/make_golden_eventvis.py from the reference's plot_event_cnt) bit for bit; the rank law the library implements
equals np.percentile's; the C ABI, the binding and the header agree; the reference's import path resolves without matplotlib
or cv2; nothing accepts a CPU tensor; the command line knows --event_png.  No compute calls: there is no GPU here."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ebfi_amd import _native as N

import eventvis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("t1x3", "t5x7", "sparse16x24", "dense8x12", "zeros6x8", "const6x8", "negmax8x12", "posmax8x12", "reals16x24",
         "sparse136x200")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "eventvis_small.npz"))


def test_fixture_holds_every_case_in_all_eight_modes(golden):
    assert len(R.MODES) == 8
    assert sorted(k[:-4] for k in golden.files if k.endswith("__in")) == sorted(CASES)
    for name in CASES:
        x = golden[name + "__in"]
        assert x.dtype == np.float32 and x.ndim == 3 and x.shape[2] == 2
        for mode in R.MODES:
            y = golden[R.mode_key(name, *mode)]
            assert y.dtype == np.uint8 and y.shape == x.shape[:2] + (3,)


def test_fixture_cases_exercise_what_they_are_for(golden):
    """The properties the case list promises, read off the data with np.percentile itself."""
    pct = lambda name, k, q: np.percentile(golden[name + "__in"][:, :, k], q)
    lo, hi, v = R.percentile32(golden["dense8x12__in"][:, :, 0], 99)
    assert (lo, hi) == (8.0, 10.0) and v == np.float32(8.100006) and v != np.float32(8.1)       # the interpolation is live
    assert R.percentile_rank(35, 99)[2] not in (0.0, 1.0)                                      # fractional index at 5 x 7
    for k in (0, 1):
        lo, hi, _ = R.percentile32(golden["sparse16x24__in"][:, :, k], 99)
        assert lo == hi                                                                        # equal neighbours
    assert golden["sparse16x24__in"].max() == 40.0                                             # the hot pixel
    assert not golden["zeros6x8__in"].any()
    c = golden["const6x8__in"]
    assert (c[:, :, 0] == 5.0).all() and pct("const6x8", 1, 99) < 5.0 and c[:, :, 1].any()
    assert pct("negmax8x12", 0, 99) < pct("negmax8x12", 1, 99) and pct("posmax8x12", 0, 99) > pct("posmax8x12", 1, 99)
    r = golden["reals16x24__in"]
    assert all(np.unique(r[:, :, k]).size == 384 for k in (0, 1)) and (r < 0).any() and (r > 1).any()
    assert ((np.abs(r) < np.finfo(np.float32).tiny) & (r != 0)).sum() == 3                     # denormals
    keys = r.view(np.uint32)
    assert all(np.unique(keys >> s).size > 8 for s in (21, 10))                                # every radix digit varies
    big = golden["sparse136x200__in"]
    assert big.shape[0] * big.shape[1] > 4096 * 4 and big.shape[1] % 4 == 0                    # more than one workgroup's slice


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_reproduces_the_reference(golden, name):
    x = golden[name + "__in"]
    for scheme, black, norm in R.MODES:
        keep = x.copy()
        got = R.plot_event_cnt_numpy(x, color_scheme=scheme, is_black_background=black, is_norm=norm)
        assert np.array_equal(x, keep)                       # (the reference writes into its input; the restatement must not)
        want = golden[R.mode_key(name, scheme, black, norm)]
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, scheme, black, norm, int((got != want).sum()))


def test_restatement_use_opencv_omits_the_reversal(golden):
    x = golden["dense8x12__in"]
    a = R.plot_event_cnt_numpy(x, "blue_red", use_opencv=False, is_black_background=False)
    b = R.plot_event_cnt_numpy(x, "blue_red", use_opencv=True, is_black_background=False)
    assert np.array_equal(a, b[:, :, ::-1]) and not np.array_equal(a, b)


@pytest.mark.parametrize("n", [1, 2, 3, 35, 96, 101, 384, 27200, 65536, 921600])
def test_rank_law_equals_np_percentile(n):
    """Distinct, exactly representable float32 values: both neighbours and the returned value, exactly."""
    from ebfi_amd.eventvis import percentile_rank
    rng = np.random.default_rng(n)
    a = (4 * rng.permutation(n)).astype(np.float32)
    s = np.sort(a)
    for q in (1, 99):
        lo, hi, g = percentile_rank(n, q)
        assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and isinstance(g, np.float32)
        want = np.percentile(a, q)
        assert isinstance(want, np.float32)
        assert R.lerp32(s[lo], s[hi], g) == want, (n, q, lo, hi, g)
        # the neighbours themselves: numpy's 'lower' and 'higher' methods return the two order statistics it interpolates
        # (an integral virtual index is its own 'higher'; the upper neighbour then carries the weight 0)
        assert s[lo] == np.percentile(a, q, method="lower"), (n, q, lo)
        assert s[hi if g != 0 else lo] == np.percentile(a, q, method="higher"), (n, q, hi)
        if lo != hi:
            # the weight alone: on the pair (0, 1) the interpolation returns it (t < 0.5) or 1 - (1 - t)
            b = np.zeros(n, np.float32)
            b[np.argsort(a)[hi:]] = 1.0
            assert np.percentile(b, q) == R.lerp32(0.0, 1.0, g)


def test_weight_is_formed_in_single_precision():
    lo, hi, g = __import__("ebfi_amd.eventvis", fromlist=["x"]).percentile_rank(96, 99)
    assert (lo, hi) == (94, 95) and g == np.float32(0.05000305) and g != np.float32(0.05)
    a = np.arange(96, dtype=np.float32)
    a[94], a[95] = 8.0, 10.0
    a[:94] = np.minimum(a[:94], 7.0)
    assert np.percentile(a, 99) == np.float32(8.100006) == R.lerp32(8.0, 10.0, g)


def test_new_symbols_are_declared_bound_and_exported():
    new = {"ebfi_event_cnt_image_workspace", "ebfi_event_cnt_image"}
    assert new <= set(N.declared_symbols()) and new <= set(N.SIGNATURES)
    if not os.path.exists(N.LIB_PATH):
        N.build()
    h = ctypes.CDLL(N.LIB_PATH)
    for name in new:
        assert hasattr(h, name), name
    header = open(os.path.join(ROOT, "include", "ebfi_hip.h")).read()
    assert "#define EBFI_ABI_VERSION 14" in header                      # a pure addition: the generation stays
    lib = N.lib()
    assert lib.ebfi_abi_version() == 14 == N.ABI_VERSION
    # the workspace query is pure host arithmetic: per plane three passes' histograms (2048 + 4 * 2048 + 4 * 1024 counters),
    # two prefix / rank tables of four targets and two percentiles; nothing without normalisation, for n == 0 or a bad shape
    per_plane = (2048 + 4 * 2048 + 4 * 1024 + 2 * 8 + 2) * 4
    assert lib.ebfi_event_cnt_image_workspace(16, 720, 1280, 1) == 32 * per_plane
    assert lib.ebfi_event_cnt_image_workspace(3, 5, 7, 1) == 6 * per_plane
    assert lib.ebfi_event_cnt_image_workspace(16, 720, 1280, 0) == 0
    assert lib.ebfi_event_cnt_image_workspace(0, 8, 8, 1) == 0
    assert lib.ebfi_event_cnt_image_workspace(1, 0, 8, 1) == 0 and lib.ebfi_event_cnt_image_workspace(-1, 8, 8, 1) == 0


def test_argument_errors_do_not_touch_the_gpu():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    lib = N.lib()
    st = (ctypes.c_int64 * 3)(128, 64, 8)
    p = ctypes.c_void_p(256)           # never dereferenced: every call below is refused before a launch
    assert lib.ebfi_event_cnt_image(None, st, 1, 8, 8, 0, 0, 1, 0, p, p, 1 << 20, None) == -1
    assert b"null" in lib.ebfi_last_error()
    assert lib.ebfi_event_cnt_image(p, st, 1, 8, 8, 0, 0, 1, 0, None, p, 1 << 20, None) == -1
    assert lib.ebfi_event_cnt_image(p, None, 1, 8, 8, 0, 0, 1, 0, p, p, 1 << 20, None) == -1
    assert lib.ebfi_event_cnt_image(p, st, -1, 8, 8, 0, 0, 1, 0, p, p, 1 << 20, None) == -1
    assert lib.ebfi_event_cnt_image(p, st, 1, 0, 8, 0, 0, 1, 0, p, p, 1 << 20, None) == -1
    assert lib.ebfi_event_cnt_image(p, st, 1, 8, 0, 0, 0, 1, 0, p, p, 1 << 20, None) == -1
    assert lib.ebfi_event_cnt_image(p, st, 1, 8, 8, 2, 0, 1, 0, p, p, 1 << 20, None) == N.EBFI_ERR_UNSUPPORTED
    assert b"gray" in lib.ebfi_last_error()
    assert lib.ebfi_event_cnt_image(p, st, 1, 8, 8, 7, 0, 1, 0, p, p, 1 << 20, None) == -1
    need = lib.ebfi_event_cnt_image_workspace(1, 8, 8, 1)
    assert lib.ebfi_event_cnt_image(p, st, 1, 8, 8, 0, 0, 1, 0, p, p, need - 1, None) == -4
    assert lib.ebfi_event_cnt_image(p, st, 1, 8, 8, 0, 0, 1, 0, p, None, 0, None) == -4
    assert lib.ebfi_event_cnt_image(p, st, 0, 8, 8, 0, 0, 1, 0, p, None, 0, None) == 0      # n == 0: nothing to do


def test_reference_import_path_needs_no_plotting_stack():
    code = ("import sys\n"
            "class Block:\n"
            "    def find_spec(self, name, path=None, target=None):\n"
            "        if name.split('.')[0] in ('matplotlib', 'cv2', 'open3d', 'mpl_toolkits'):\n"
            "            raise ImportError('blocked: ' + name)\n"
            "sys.meta_path.insert(0, Block())\n"
            "sys.path.insert(0, %r)\n"
            "from myutils.vis_events.matplotlib_plot_events import event_visualisation\n"
            "import inspect\n"
            "v = event_visualisation()\n"
            "sig = inspect.signature(v.plot_event_cnt)\n"
            "assert list(sig.parameters) == ['event_cnt', 'is_save', 'path', 'color_scheme', 'use_opencv', 'is_black_background', 'is_norm']\n"
            "d = {k: p.default for k, p in sig.parameters.items()}\n"
            "assert (d['path'], d['color_scheme'], d['use_opencv'], d['is_black_background'], d['is_norm']) == (None, 'green_red', False, True, True)\n"
            "sig = inspect.signature(v.plot_frame)\n"
            "assert list(sig.parameters) == ['frame', 'is_save', 'path', 'cmap'] and sig.parameters['cmap'].default == 'gray'\n"
            "assert not {'matplotlib', 'cv2', 'open3d'} & set(sys.modules)\n"
            "print('ok')\n" % os.path.join(ROOT, "ebfi-be_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_cpu_input_is_refused():
    from ebfi_amd.eventvis import event_count_images
    from myutils.vis_events.matplotlib_plot_events import event_visualisation
    with pytest.raises(NotImplementedError):
        event_count_images(torch.zeros(1, 2, 4, 4))
    with pytest.raises(NotImplementedError):
        event_visualisation().plot_event_cnt(np.zeros((4, 4, 2), np.float32), is_save=False)
    with pytest.raises(NotImplementedError):
        event_visualisation().plot_event_cnt(torch.zeros(4, 4, 2), is_save=False, color_scheme="blue_red")


def test_plot_frame_writes_the_array(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from myutils.vis_events.matplotlib_plot_events import event_visualisation
    frame = np.random.default_rng(0).integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    path = str(tmp_path / "f.png")
    event_visualisation().plot_frame(frame, is_save=True, path=path)
    assert np.array_equal(np.asarray(Image.open(path)), frame)


def test_infer_cli_lists_event_png():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "ebfi-be_amd", "infer_ours.py"), "--help"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--event_png" in r.stdout
