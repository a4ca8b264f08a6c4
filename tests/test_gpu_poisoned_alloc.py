"""The suite's reference comparisons, run again with every new device buffer poisoned (tests/poison.py: 0xFF bytes, NaN as a
float, -1 as an integer).

Every native op takes its outputs and workspaces from torch.empty / empty_like / new_empty.  In a fresh test process that memory
is nearly always zero, so a kernel that adds up a partial nobody wrote -- a slice of a plane with no elements, a tile past the
ragged edge, a round of samples that never ran -- still gets the right sum, and "the same bits twice" holds because both runs
read the same zeros.  Under the caching allocator of a long training run the same read returns whatever the block held before.
Here the comparisons the suite already trusts (float64, the CPU oracle, golden fixtures: the existing test functions, called
with explicit arguments, or a closure that applies the other module's own check helper) run inside `poisoned_allocations()`.
No new reference and no new tolerance: a case asserts what the wrapped test asserts, and that the patch saw at least one
device allocation (else it missed the wrapper and proved nothing).

CASES carries per case the ebfi_amd modules whose allocations it reaches, as data: tests/test_poison_host.py holds the table
against the package source (every module that allocates is in a case or in EXEMPT) without importing any device code.

The module-level workspace caches (loss, metrics, eventvis) are emptied before a case runs, so that the workspace is allocated
again, poisoned; a cached one from an earlier test of the process would stay as clean as that test left it.

INTEGER WORKSPACES.  A garbage count, key or index read before it is written is an out-of-bounds access, so these were settled
by reading csrc/*.hip before any of their cases ran.  Field by field (a write: a kernel or a hipMemsetAsync inside the entry
point, before the first read on the same stream):

  encodings.hip, ebfi_events_to_grid / ebfi_interpolate_to_image (workspace `Layout`)
    keys[0]        grid_keys / bilinear_keys write all n entries; keys[1], perm[0..1]: sort_scatter writes all n slots of the
                   other buffer every pass (the table counts exactly the n active entries), pass 0 reads no permutation
    hist           sort_hist writes all 256 * nb words (every thread of every workgroup stores its bin) before scan_tiles
    sums           scan_tiles writes one word per tile (nt workgroups) before scan_sums and sort_scatter read them
    seg            grid_segments writes seg[0 .. nkeys]; the accumulation reads seg[pix], seg[pix + 1] with pix < nkeys
    bounds         grid_bounds writes 2 * bins words; read only by the naive-voxel instance, which that launch precedes
    pxs pys dxs dys ws   bilinear_prepare writes all n entries before bilinear_keys / bilinear_accumulate
    out            memset for n == 0, short lists and the bilinear image (which accumulates onto it); else every (plane, pixel)
  events.hip, ebfi_events_to_stack: bounds[0 .. 2 * bins] all written by events_bounds (bi <= bins); used in comparisons only;
    out memset first
  iwe.hip (`Layout`, `IndexLayout`; the sort is the one above): keys[0] by warp_events / interpolate_keys / source_keys /
    gather_keys for every entry sorted; idx (the destination keys), src, pol by warp_events for all B * N events; w likewise;
    seg, seg2 by run_starts for k in [0, B * P]; keys2 / perm2 by gather_keys and the three sorts in turn (each reads the buffer
    the pass before it wrote: radix_sort starts at *cur); partials by loss_partials, one per workgroup, before loss_final.
    The gradient's index: ebfi_iwe_source_index fills perm[cur] and seg (N == 0: seg memset, perm unread), and
    ebfi_iwe_warping_backward derives the same `cur` from key_passes(B * P); EventWarping.forward always builds it first.
  esim.hip: counts[k][p] written by esim_walk<count> for every k < n, p < H * W before the host's cumsum; the offsets come from
    it; every store of esim_walk<emit> is guarded by `e < capacity`; state written whole by esim_init
  eventvis.hip: the histograms of all planes and passes are memset per call; select<0> / select<1> write {prefix, rank} of all
    four targets (the total of the scanned bins exceeds every rank) before hist<1> / hist<2> and select<1> / select<2> read
    them; the two percentiles by select<2> before eventvis_colour.  Whatever the state words held, every index formed from
    them is alias_of(...) in [0, 3] times a constant: no garbage can leave the plane's table.
  blur.hip: no integer field; the scratch plane of frame2dcp is written whole by the row pass before the column pass
  bcloss.hip (the same sort): keys[0] and val by scatter_entries, four entries for every one of the K pixels, in the backward
    kernel that precedes the sort; seg by run_starts for k in [0, K]
  telemetry.hip: hist zeroed by stats_zero (all S * nb words) before stats_chunk adds; the chunk records stats_finish reads
    (first .. first + count) are exactly those the workgroups with a segment wrote; offsets are clamped on the device

Nothing was found unwritten, so all of them are in the table.  The other byte workspaces (conv, fac, dcn, rc_fused, wgradqueue,
fused, norm) hold floats and doubles only; dcn.hip's integer cells are LDS; the `flags` words of the LPIPS workspaces are
booleans that are OR-ed, never an index.
"""
import importlib
import os

import pytest
import torch

from poison import poisoned_allocations

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _mod(name):
    return importlib.import_module(name)


def call(module, test, *args, **kwargs):
    """The existing test `module.test`, called with explicit arguments.  An argument that is a function is evaluated first
    (with the fixture getter): values that only exist once the other module is imported, and this module's fixtures."""
    def run(fx):
        resolve = lambda a: a(fx) if callable(a) else a
        getattr(_mod(module), test)(*[resolve(a) for a in args], **{k: resolve(v) for k, v in kwargs.items()})
    return run


def fixture(name):
    return lambda fx: fx(name)


def by_id(module, cid, table="CASES"):
    return lambda fx: next(c for c in getattr(_mod(module), table) if c.id == cid)


def _drop_cached_workspaces():
    from ebfi_amd import eventvis, loss, metrics
    for cache in (loss._cb_workspaces, loss._dh_workspaces, metrics._workspaces, eventvis._workspaces):
        cache.clear()


# ------------------------------------------------------------------------------------------------------------------ closures
def metrics_case(N, C, H, W):
    """frame_metrics at a size the parameter list of test_gpu_metrics does not hold, under that module's own _check."""
    def run(fx):
        M = _mod("test_gpu_metrics")
        from ebfi_amd.metrics import frame_metrics
        pred, target = M._pair(N, C, H, W, seed=H * 1000 + W + N + C)
        M._check(frame_metrics(pred.cuda(), target.cuda()), pred, target)
    return run


def psroi_case(name):
    """test_gpu_dcn_pooling keeps its device results in an lru_cache: run the fixture again, then that module's comparisons."""
    def run(fx):
        P = _mod("test_gpu_dcn_pooling")
        import numpy as np
        c = P.K.case(name)
        out, count, gi, gt = P.run_device(c)
        assert np.array_equal(count.cpu().numpy(), P.oracle(name, P.F32)[1])
        _, _, want_gi, want_gt = P.oracle(name, P.F64)
        assert P._relnp(out, P.oracle(name, P.F64)[0]) < P.FWD_BAR
        assert P._relnp(gi, want_gi) < P.GRAD_BAR
        if c.no_trans:
            assert gt.numel() == 0
        else:
            assert P._relnp(gt, want_gt) < P.GRAD_BAR
    return run


def loss_f64_case(name):
    """test_gpu_loss_f64 keeps one device run per case in `_runs`: drop it, so that the run happens here."""
    def run(fx):
        L = _mod("test_gpu_loss_f64")
        L._runs.pop(name, None)
        try:
            L.test_sign_field_against_float64(name)
            L.test_adjoint_of_the_devices_own_field(name)
            L.test_value_against_float64(name)
        finally:
            L._runs.pop(name, None)                 # (the module's own tests make their own, unpoisoned run)
    return run


def lpips_alex_forward(fx):
    L = _mod("test_gpu_lpips")
    from ebfi_amd.lpips import load_alex_lpips
    lin_path, backbone_path, trunk = fx("alex_weights")
    alex = load_alex_lpips(lin_path, backbone_path, device="cuda"), trunk, (lin_path, backbone_path)
    for n, c, h, w, kind in [(1, 3, 31, 31, "random"), (16, 1, 31, 31, "unclamped")]:
        L.test_lpips_matches_the_restatement(alex, n, c, h, w, kind)


def lpips_vgg_forward(fx):
    L = _mod("test_gpu_lpips_vgg")
    from ebfi_amd.lpips import load_vgg_lpips
    lin_path, backbone_path, _ = fx("vgg_weights")
    L.test_lpips_vgg_matches_the_restatement(load_vgg_lpips(lin_path, backbone_path, device="cuda"), fx("vgg_yardstick"), (1, 3, 16, 16, "random"))


def lpips_alex_gradient(fx):
    L = _mod("test_gpu_lpips_alex_grad")
    from ebfi_amd.lpips import load_alex_lpips
    lin_path, backbone_path, _ = fx("alex_weights")
    model = load_alex_lpips(lin_path, backbone_path, device="cuda", train=True)
    L.test_gradient_matches_float64_autograd(model, None, fx("alex_grad_yardstick"), (1, 3, 31, 31, "random"))


def lpips_vgg_gradient(fx):
    L = _mod("test_gpu_lpips_vgg_grad")
    from ebfi_amd.lpips import load_vgg_lpips
    lin_path, backbone_path, _ = fx("vgg_weights")
    model = load_vgg_lpips(lin_path, backbone_path, device="cuda")
    L.test_gradient_matches_float64_autograd(model, None, fx("vgg_grad_yardstick"), (1, 3, 16, 16, "random"))


def charbonnier(fx):
    V = _mod("test_gpu_validation")
    V.test_charbonnier_forward_matches_float64()
    V.test_charbonnier_backward_matches_float64_autograd()


def duty_head(name):
    """The cases of test_gpu_exposure are cached with their device tensors (inputs only): both directions of one case."""
    def run(fx):
        X = _mod("test_gpu_exposure")
        X.test_duty_head_forward_vs_float64(name)
        X.test_duty_head_backward_vs_float64(name)
    return run


def model_train_step(fx):
    """test_gpu_model's `mode` fixture sets the compute mode around the test: the same here."""
    from ebfi_amd import conv
    conv.set_compute_dtype("bf16x3")
    try:
        _mod("test_gpu_model").test_train_step_vs_oracle(fx("model_fix"), "bf16x3")
    finally:
        conv.set_compute_dtype("fp32")


# ------------------------------------------------------------------------------------------------------------------ the table
# the smallest existing parameter set per convolution route with a ragged last tile (tests/conv_routes_ref.py names the kernels)
ROUTES = [
    "a_x_fp32_k3_leaky_le32", "a_x_fp32_k3_sigmoid_gt32", "a_x_fp32_k7_leaky_le32", "a_x_fp32_k3s2_leaky",
    "a_x_x3_k3_sigmoid_v1_ragged", "a_x_x3_k3_leaky_v4_mt1", "a_x_x3_k3_leaky_v1_mt2", "a_x_x3_k1_sigmoid_v1_mt1",
    "a_wb_fp32_k3_leaky", "a_wb_x3_k3_leaky", "a_wb_x3ws_k3_leaky", "a_wb_bf16_k3_leaky", "a_wb_fp32_k1_none",
    "a_wb_fp32_k7_sigmoid", "a_wb_fp32_k3s2_sigmoid", "a_wb_fp32_k7s2_leaky", "a_wb_x3_k7_sigmoid", "a_wb_x3_k3_small_wg_leaky",
    "a_wb_fp32_thin_in_leaky", "a_wb_fp32_thin_ins2_sigmoid", "a_wb_x3_shift_in_leaky", "a_wb_x3_shift_in_dword_leaky",
    "b_fp32_k3s1p0", "b_fp32_k3s2p2", "b_fp32_k7s2p2", "b_bf16x3_k3s1p2", "b_bf16x3_k7s1p5", "b_bf16x3_k3s1p3", "b_bf16_k3s1p2",
    "b_bank_k3s1p3", "c_x3_ws_aligned", "c_x3_shift_misaligned_g_gpout", "c_bank_c48_misaligned_x", "c_fp32_channel_slice",
    "d_bf16x3_grad_preact", "e_wb_f16_tr_leaky", "e_wb_f16_ws_leaky", "e_x_f16_none", "e_x_x3_leaky_folded",
]
CONV = ("conv", "weightbank")
CASES = [("conv-route-" + cid, CONV, call("test_gpu_conv_routes", "test_route", cid)) for cid in ROUTES]
CASES += [
    # ---- conv.py: forward, data gradient, weight gradient through ConvBiasAct (fp32), thin / shift kernels, fp16 backward
    ("conv-fp32-ragged", CONV, call("test_gpu_conv", "test_conv_forward_backward_vs_cpu", 1, 128, 13, 70, 64, 3, 1, 1, 1, True)),
    ("conv-fp32-s2-odd", CONV, call("test_gpu_conv", "test_conv_forward_backward_vs_cpu", 2, 12, 33, 47, 20, 3, 2, 1, 0, False)),
    ("conv-fp32-7x7-s2", CONV, call("test_gpu_conv", "test_conv_forward_backward_vs_cpu", 1, 6, 10, 12, 8, 7, 2, 3, 1, False)),
    ("conv-fp32-7x7-direct", CONV, call("test_gpu_conv", "test_conv_forward_backward_vs_cpu", 2, 5, 9, 41, 4, 7, 1, 3, 0, False)),
    ("conv-fp32-tiny-map", CONV, call("test_gpu_conv", "test_conv_forward_backward_vs_cpu", 2, 8, 2, 2, 8, 3, 1, 1, 1, True)),
    ("conv-thin-out-fp32", CONV, call("test_gpu_conv", "test_thin_layer_weight_gradients_vs_cpu", 2, 32, 128, 256, 1, 3, 1, 1, 0, True, "out", "fp32")),
    ("conv-thin-ins2-fp32", CONV, call("test_gpu_conv", "test_thin_layer_weight_gradients_vs_cpu", 6, 4, 200, 256, 16, 3, 2, 1, 0, True, "ins2", "fp32")),
    ("conv-shift-out-x3", CONV, call("test_gpu_conv", "test_thin_layer_weight_gradients_vs_cpu", 3, 64, 130, 172, 3, 3, 1, 1, 2, True, "out", "bf16x3")),
    ("conv-shift-out7-x3", CONV, call("test_gpu_conv", "test_thin_layer_weight_gradients_vs_cpu", 3, 16, 150, 230, 3, 7, 1, 0, 0, False, "out7", "bf16x3")),
    ("conv-shift-in-x3", CONV, call("test_gpu_conv", "test_thin_layer_weight_gradients_vs_cpu", 2, 4, 136, 250, 64, 3, 1, 1, 1, True, "in", "bf16x3")),
    ("conv-x3-vs-fp32", CONV, call("test_gpu_conv", "test_bf16x3_split_precision_mode_vs_fp32_reference", 1, 20, 17, 33, 24, 3, 0)),
    ("conv-7x7-s2-dgrad-parity", CONV, call("test_gpu_conv", "test_stride2_7x7_data_gradient_by_parity_vs_cpu", 1, 3, 37, 51, 20, 3, 0)),
    ("conv-packed-grouped", CONV, call("test_gpu_conv", "test_packed_grouped_conv_with_epilogue_extras_vs_cpu")),
    ("conv-f16-backward-ragged", CONV + ("f16scale",), call("test_gpu_conv", "test_fp16_backward_kernels_vs_cpu", 1, 128, 13, 38, 64, 1, 1.0, 1.0)),
    ("conv-f16-backward-c48", CONV + ("f16scale",), call("test_gpu_conv", "test_fp16_backward_kernels_vs_cpu", 2, 48, 16, 32, 32, 1, 1.0, 1.0)),
    ("conv-f16-backward-c32", CONV + ("f16scale",), call("test_gpu_conv", "test_fp16_backward_kernels_vs_cpu", 1, 32, 32, 32, 48, 0, 1.0, 1.0)),
    ("conv-shuffle-forward", CONV, call("test_gpu_conv_shuffle", "test_split_precision_forward_stores_through_the_shuffle", 1, 64, 13, 36, 128, 0)),
    ("conv-shuffle-forward-small", CONV, call("test_gpu_conv_shuffle", "test_split_precision_forward_stores_through_the_shuffle", 2, 32, 6, 8, 64, 1)),
    ("conv-shuffle-dgrad", CONV, call("test_gpu_conv_shuffle", "test_data_gradient_stores_masked_through_the_inverse_shuffle", 1, 128, 14, 36, 64, False)),
    ("conv-shuffle-dgrad-image", CONV + ("c16",), call("test_gpu_conv_shuffle", "test_data_gradient_stores_masked_through_the_inverse_shuffle", 2, 64, 32, 132, 96, True)),
    ("conv-shuffle-head", CONV + ("model",), call("test_gpu_conv_shuffle", "test_reconstruction_head_as_one_node", 2, 64, 16, 32, True)),
    # ---- c16.py: the writers of the fp16 images
    ("c16-to-c16-masked", ("c16",), call("test_gpu_c16", "test_to_c16_matches_torch", 1, 128, 13, 36, True)),
    ("c16-to-c16-one-quad", ("c16",), call("test_gpu_c16", "test_to_c16_matches_torch", 3, 16, 8, 4, False)),
    ("c16-cat2-ragged", ("c16",), call("test_gpu_c16", "test_image_of_a_concatenation_from_its_two_parts", 1, 8, 24, 13, 36)),
    ("c16-cat2-one-quad", ("c16",), call("test_gpu_c16", "test_image_of_a_concatenation_from_its_two_parts", 3, 40, 8, 8, 4)),
    ("c16-forward-epilogue", ("c16", "conv"), call("test_gpu_c16", "test_forward_conv_writes_the_image_of_its_output", 1, 64, 13, 36, 128, 2)),
    ("c16-dgrad-images", ("c16", "conv"), call("test_gpu_c16", "test_data_gradient_reads_and_writes_images", 1, 64, 13, 36, 128, 2, True)),
    ("c16-wgrad-from-images", ("c16", "conv"), call("test_gpu_c16", "test_weight_gradient_from_images", 1, 64, 13, 36, 128, 2)),
    ("c16-wgrad-batched", ("c16", "conv"), call("test_gpu_c16", "test_batched_weight_gradients_equal_the_single_launches", 2, 37, 100, 2)),
    ("c16-wgrad-writes-gpre-image", ("c16", "conv"), call("test_gpu_c16", "test_weight_gradient_writes_the_image_of_the_preactivation_gradient", 1, 48, 13, 36, 32)),
    ("c16-rc-stages-write-images", ("c16", "rc_fused"), call("test_gpu_c16", "test_fused_residual_control_stages_write_images")),
    ("c16-rc-tail-epilogue", ("c16", "conv"), call("test_gpu_c16", "test_residual_control_tail_in_the_convolution_epilogue", 1, 64, 13, 36)),
    ("c16-planar-filters", ("c16", "conv"), call("test_gpu_c16", "test_conv_writes_planar_fp16_filters_only", 1, 64, 13, 36, 64)),
    ("c16-planar-gradients", ("c16", "conv"), call("test_gpu_c16", "test_backward_convs_stage_planar_fp16_gradients", 1, 64, 24, 68, 64)),
    ("c16-storage-vs-cpu", ("c16", "conv"), call("test_gpu_c16", "test_storage_kernels_against_cpu_fp32_autograd", 1, 64, 24, 68, 64)),
    # ---- the batched weight gradients and the deferred queue
    ("wgrad-multi-bias", ("conv", "wgradqueue"), call("test_gpu_wgrad_multi", "test_multi_matches_float64_and_the_single_layer_launch", fixture("four"), True)),
    ("wgrad-multi-no-bias", ("conv", "wgradqueue"), call("test_gpu_wgrad_multi", "test_multi_matches_float64_and_the_single_layer_launch", fixture("four"), False)),
    ("wgrad-multi-seventeen", ("conv", "wgradqueue"), call("test_gpu_wgrad_multi", "test_seventeen_items_take_two_launches", None)),
    ("wgrad-queue-scope", ("wgradqueue", "conv", "weightbank"), call("test_gpu_wgrad_queue", "test_backward_outside_a_scope_launches_the_single_layer_kernels")),
    # ---- fused.py
    ("fused-scale-residual-cat-4", ("fused",), call("test_gpu_model", "test_scale_residual_cat_stage_vs_float64", 2, 3, 1, 4)),
    ("fused-scale-residual-cat-12", ("fused",), call("test_gpu_model", "test_scale_residual_cat_stage_vs_float64", 1, 6, 3, 4)),
    ("fused-scale-residual-cat-1028", ("fused",), call("test_gpu_model", "test_scale_residual_cat_stage_vs_float64", 2, 4, 4, 257)),
    ("fused-scale-residual-cat-pair", ("fused",), call("test_gpu_model", "test_scale_residual_cat_kernel_pair")),
    ("fused-scale-cat", ("fused",), call("test_gpu_model", "test_scale_cat_stage_of_exposure_decision")),
    ("fused-scalar-conv-bank", ("fused",), call("test_gpu_scalar_conv", "test_scalar_conv_bank_matches_torch", 3, 5, 2, 16, False)),
    ("fused-scalar-conv-bank-s32", ("fused",), call("test_gpu_scalar_conv", "test_scalar_conv_bank_matches_torch", 32, 1, 8, 48, True)),
    ("fused-scalar-conv-grid", ("fused",), call("test_gpu_scalar_conv_grid", "test_scalar_conv_backward_grid_matches_float64", 12, 8, 8, 100)),
    ("fused-product-mean", ("fused",), call("test_gpu_model", "test_product_mean_stage")),
    ("fused-ed-head-2-slices", ("fused",), call("test_gpu_edhead", "test_ed_head_regime_shapes", (1, 4, 2, 91, 92), "m16_s1")),
    ("fused-ed-head-3-slices", ("fused",), call("test_gpu_edhead", "test_ed_head_regime_shapes", (1, 4, 2, 106, 116), "m0.4_s1.5")),
    ("fused-ed-head-hw4", ("fused",), call("test_gpu_edhead", "test_ed_head_regime_shapes", (3, 6, 3, 2, 2), "m16_s1")),
    ("fused-ed-head-9-samples", ("fused",), call("test_gpu_edhead", "test_ed_head_regime_shapes", (9, 8, 4, 4, 8), "m0.4_s1.5")),
    ("fused-ed-head-vs-torch", ("fused",), call("test_gpu_model", "test_exposure_decision_head_vs_torch_cpu")),
    ("fused-ed-fallback-pair", ("fused", "norm"), call("test_gpu_edhead", "test_fallback_pair_conditioning_sweep", "m16_s1")),
    ("fused-reflect-pad-backward", ("fused",), call("test_gpu_fac", "test_deterministic_pad_adjoints_match_torch", "reflect", 3)),
    ("fused-replicate-pad-backward", ("fused",), call("test_gpu_fac", "test_deterministic_pad_adjoints_match_torch", "replicate", 2)),
    # ---- rc_fused.py (the _ex halves form of scale_residual_cat runs inside it: rc_fused.py, the two ebfi_scale_residual_cat_*_ex calls)
    ("rc-fused-equals-layerwise", ("rc_fused", "weightbank", "conv", "fused"), call("test_gpu_model", "test_fused_residual_control_equals_layerwise")),
    ("rc-fused-f64-two-rounds-book", ("rc_fused", "weightbank", "c16", "f16scale"),
     call("test_gpu_residual_control", "test_residual_control_vs_float64", by_id("test_gpu_residual_control", "a-64-s2-b2-2x4"), "book", 0.01)),
    ("rc-fused-f64-ragged-book", ("rc_fused", "weightbank", "c16", "f16scale"),
     call("test_gpu_residual_control", "test_residual_control_vs_float64", by_id("test_gpu_residual_control", "b-64-s1-b1-37x100"), "book", 1.0)),
    ("rc-fused-f64-w-not-quads-bank", ("rc_fused", "weightbank"),
     call("test_gpu_residual_control", "test_residual_control_vs_float64", by_id("test_gpu_residual_control", "a-64-s2-b1-2x6"), "bank", 0.01)),
    # ---- fold3d.py: the SE gate in both forms (70 samples: the rounds of grad_W / grad_b; 288 channels; 64 x 96: two slices),
    #      one detail-branch stage
    ("fold3d-se-gate", ("fold3d", "model"), call("test_gpu_model", "test_se_gate_kernels_vs_torch_cpu")),
    ("fold3d-se-gate-shuffled", ("fold3d", "model"), call("test_gpu_model", "test_se_gate_through_the_pixel_shuffle_vs_torch_cpu")),
    ("fold3d-detail-block-48", ("fold3d", "conv", "model"), call("test_gpu_detail_stages", "test_stage_vs_float64_module", by_id("test_gpu_detail_stages", "block-48-5x6"), "bf16x3")),
    ("fold3d-detail-block-s2-book", ("fold3d", "conv", "model", "weightbank"),
     call("test_gpu_detail_stages", "test_stage_vs_float64_module", by_id("test_gpu_detail_stages", "block-16to24-s2-9x7"), "book")),
    ("fold3d-detail-stem", ("fold3d", "conv", "model"), call("test_gpu_detail_stages", "test_stage_vs_float64_module", by_id("test_gpu_detail_stages", "stem-16-9x7"), "fp32")),
    # ---- fac.py: tile, generic and fp16-plane routes
    ("fac-tile-ragged", ("fac",), call("test_gpu_fac", "test_forward_backward_vs_oracle", 2, 2, 9, 132, 5)),
    ("fac-tile-narrow", ("fac",), call("test_gpu_fac", "test_forward_backward_vs_oracle", 2, 3, 7, 12, 5)),
    ("fac-generic-w-not-quads", ("fac",), call("test_gpu_fac", "test_forward_backward_vs_oracle", 1, 2, 6, 10, 5)),
    ("fac-generic-k7", ("fac",), call("test_gpu_fac", "test_forward_backward_vs_oracle", 1, 1, 4, 8, 7)),
    ("fac-backward-tail-lane", ("fac",), call("test_gpu_fac", "test_forward_backward_vs_oracle", 1, 5, 33, 260, 5)),
    ("fac-strided", ("fac",), call("test_gpu_fac", "test_strided_layouts_any_stride")),
    ("fac-activation-mask", ("fac",), call("test_gpu_fac", "test_backward_with_filter_activation_mask")),
    ("fac-p16", ("fac", "f16scale"), call("test_gpu_c16", "test_fac_on_fp16_filter_planes", 2, 3, 9, 36)),
    ("fac-p16-ragged", ("fac", "f16scale"), call("test_gpu_c16", "test_fac_on_fp16_filter_planes", 1, 64, 24, 132)),
    ("fac-fused-kernelconv-ragged", ("fac", "conv", "weightbank"), call("test_gpu_fac", "test_fused_kernelconv_fac_vs_unfused_pair_and_oracle", 2, 8, 16, 20, 36)),
    ("fac-fused-kernelconv-tiny-map", ("fac", "conv", "weightbank"), call("test_gpu_fac", "test_fused_kernelconv_fac_vs_unfused_pair_and_oracle", 1, 5, 16, 9, 4)),
    # ---- dcn.py
    ("dcn-ragged", ("dcn",), call("test_gpu_dcn", "test_forward_backward_vs_oracle", lambda fx: _mod("test_gpu_dcn").CASES[1])),
    ("dcn-s2-two-co-blocks", ("dcn",), call("test_gpu_dcn", "test_forward_backward_vs_oracle", lambda fx: _mod("test_gpu_dcn").CASES[3])),
    ("dcn-sub-blocks", ("dcn",), call("test_gpu_dcn", "test_forward_backward_vs_oracle", lambda fx: _mod("test_gpu_dcn").CASES[6])),
    ("dcn-lds-window", ("dcn",), call("test_gpu_dcn", "test_forward_backward_vs_oracle", lambda fx: _mod("test_gpu_dcn").CASES[9])),
    ("dcn-smaller-than-a-tile", ("dcn",), call("test_gpu_dcn", "test_forward_backward_vs_oracle", lambda fx: _mod("test_gpu_dcn").CASES[10])),
    ("dcn-f64-protocol", ("dcn",), call("test_gpu_dcn", "test_gradients_vs_fp64_oracle_reference_protocol")),
] + [("dcn-psroi-" + name, ("dcn",), psroi_case(name)) for name in "ABCDE"] + [
    ("dcn-psroi-autograd", ("dcn",), call("test_gpu_dcn_pooling", "test_dcnv2pooling_through_autograd")),
    # ---- loss.py
    ("loss-gauss5", ("loss",), call("test_gpu_model", "test_gauss5_kernel_pair_vs_reference_conv")),
    ("loss-census", ("loss",), call("test_gpu_model", "test_census_kernel_pair_vs_slice_formulation")),
    ("loss-census-pair-7x9", ("loss",), call("test_gpu_census_pair", "test_weighted_loss_and_gradients_against_the_oracle", fixture("census_images"), 7, 9, 0.1, 1.0, True)),
    ("loss-census-pair-37x41", ("loss",), call("test_gpu_census_pair", "test_weighted_loss_and_gradients_against_the_oracle", fixture("census_images"), 37, 41, 1.0, 0.1, True)),
    ("loss-census-pair-one", ("loss",), call("test_gpu_census_pair", "test_weighted_loss_and_gradients_against_the_oracle", fixture("census_images"), 20, 37, 0.1, 1.0, False)),
    ("loss-census-pair-bits", ("loss",), call("test_gpu_census_pair", "test_pair_is_bit_equal_to_the_single_pair_entry_points", fixture("census_images"), 37, 41, 0.1, 1.0, True)),
    ("loss-laplacian-pyramid", ("loss",), call("test_gpu_model", "test_laplacian_difference_pyramid_vs_operator_formulation")),
    ("loss-laplacian-tiles-ragged", ("loss",), call("test_gpu_loss_tiles", "test_tiled_pyramid_vs_gpu_operator_formulation", 80, 112, 5, True, 3)),
    ("loss-laplacian-tiles-4x6", ("loss",), call("test_gpu_loss_tiles", "test_tiled_pyramid_vs_gpu_operator_formulation", 4, 6, 2, False, 1)),
    ("loss-laplacian-f64-ragged", ("loss",), loss_f64_case("ragged")),
    ("loss-laplacian-f64-min5", ("loss",), loss_f64_case("min5")),
    ("loss-train-loss-f64", ("loss",), call("test_gpu_loss_f64", "test_train_loss_end_to_end", 1, 32, 48, 20000, True, 2, "rand")),
    ("loss-charbonnier", ("loss",), charbonnier),                       # (holds 3 x 3 x 37 x 129: two row strips, the second ragged)
    ("loss-duty-head-37x129", ("loss",), duty_head("3x37x129")),
    ("loss-duty-head-5x7x9", ("loss",), duty_head("5x7x9")),
    ("loss-duty-head-1x1", ("loss",), duty_head("1x1")),
    # ---- lpips.py
    ("lpips-alex-forward", ("lpips",), lpips_alex_forward),
    ("lpips-vgg-forward", ("lpips",), lpips_vgg_forward),
    ("lpips-alex-gradient", ("lpips",), lpips_alex_gradient),
    ("lpips-vgg-gradient", ("lpips",), lpips_vgg_gradient),
    # ---- metrics.py: 7 x 7; two row strips by two column strips on the narrow path (49 x 130) and on the 16-byte path with a
    #      second column strip of 4 columns (52 x 132)
    ("metrics-7x7", ("metrics",), call("test_gpu_metrics", "test_kernel_vs_restatement", 7, 7, 5, 3)),
    ("metrics-37x53", ("metrics",), call("test_gpu_metrics", "test_kernel_vs_restatement", 37, 53, 16, 1)),
    ("metrics-49x130", ("metrics",), metrics_case(3, 3, 49, 130)),
    ("metrics-52x132", ("metrics",), metrics_case(3, 1, 52, 132)),
    ("metrics-strided", ("metrics",), call("test_gpu_metrics", "test_strided_views_without_copies")),
    ("metrics-narrow-path", ("metrics",), call("test_gpu_metrics", "test_unaligned_rows_take_the_narrow_path")),
    # ---- norm.py: HW = 4 (fewer elements than the 16 slices) and (1, 6, 3, 5, 4)
    ("norm-group-norm-hw4", ("norm",), call("test_gpu_edhead", "test_group_norm_alone", "hw_4", (3, 6, 3, 2, 2), True, "m16_s1")),
    ("norm-group-norm-more-groups", ("norm",), call("test_gpu_edhead", "test_group_norm_alone", "more_groups_than_channels", (5, 4, 2, 2, 4), True, "m16_s1")),
    ("norm-group-norm-no-affine", ("norm",), call("test_gpu_edhead", "test_group_norm_alone", "no_affine", (2, 8, 2, 8, 12), False, "m16_s1")),
    ("norm-group-norm-vs-torch", ("norm",), call("test_gpu_model", "test_groupnorm_kernels_vs_torch_cpu")),
    # ---- bcloss.py, iwe.py
    ("bcloss-terms-general", ("bcloss",), call("test_gpu_bc", "test_terms_against_the_float64_reference", fixture("bc_golden"), lambda fx: _mod("ebfi_amd.bcloss"), "general", "gen")),
    ("bcloss-terms-bounds-tc", ("bcloss",), call("test_gpu_bc", "test_terms_against_the_float64_reference", fixture("bc_golden"), lambda fx: _mod("ebfi_amd.bcloss"), "bounds", "tc")),
    ("bcloss-terms-pile-tv", ("bcloss",), call("test_gpu_bc", "test_terms_against_the_float64_reference", fixture("bc_golden"), lambda fx: _mod("ebfi_amd.bcloss"), "pile", "tv")),
    ("bcloss-sobel", ("bcloss",), call("test_gpu_bc", "test_sobel_forward_and_backward", fixture("bc_golden"), lambda fx: _mod("ebfi_amd.bcloss"), "border")),
    ("bcloss-odd-sizes", ("bcloss",), call("test_gpu_bc", "test_odd_sizes_against_the_float64_restatement", fixture("bc_golden"), lambda fx: _mod("ebfi_amd.bcloss"), (2, 33, 66))),
    ("bcloss-scatter-order", ("bcloss",), call("test_gpu_bc", "test_the_scatter_adds_in_the_promised_order", fixture("bc_golden"), lambda fx: _mod("ebfi_amd.bcloss"), "pile")),
] + [("iwe-images-" + name, ("iwe",), call("test_gpu_iwe", "test_images_and_indices_are_the_reference_bits", fixture("iwe_golden"), lambda fx: _mod("ebfi_amd.iwe"), name))
     for name in ("general", "pile", "bounds", "empty", "average")] + [
    ("iwe-warping-general", ("iwe",), call("test_gpu_iwe", "test_event_warping_against_the_float64_reference", fixture("iwe_golden"), lambda fx: _mod("ebfi_amd.iwe"), "general")),
    ("iwe-warping-pile", ("iwe",), call("test_gpu_iwe", "test_event_warping_against_the_float64_reference", fixture("iwe_golden"), lambda fx: _mod("ebfi_amd.iwe"), "pile")),
    ("iwe-warping-empty", ("iwe",), call("test_gpu_iwe", "test_event_warping_against_the_float64_reference", fixture("iwe_golden"), lambda fx: _mod("ebfi_amd.iwe"), "empty")),
    ("iwe-wave-walk-65", ("iwe",), call("test_gpu_iwe", "test_run_lengths_around_the_wave_walk", lambda fx: _mod("ebfi_amd.iwe"), 65)),
    # ---- the other integer workspaces (see the docstring): encodings.py, events / blur, esim.py, eventvis.py, telemetry.py
] + [("encodings-fixture-" + name, ("encodings",), call("test_gpu_encodings", "test_fixture_cases", fixture("encodings_golden"), lambda fx: _mod("ebfi_amd.encodings"), name))
     for name in ("c1", "b1", "n0", "n3", "n4", "tzero", "hot4096")] + [
    ("encodings-wave-walk-65", ("encodings",), call("test_gpu_encodings", "test_run_lengths_around_the_wave_walk", lambda fx: _mod("ebfi_amd.encodings"), 65)),
    ("encodings-bilinear", ("encodings",), call("test_gpu_encodings", "test_bilinear_images", fixture("encodings_golden"), lambda fx: _mod("ebfi_amd.encodings"))),
    ("encodings-mask", ("encodings",), call("test_gpu_encodings", "test_mask_last_writer_wins", fixture("encodings_golden"), lambda fx: _mod("ebfi_amd.encodings"))),
    ("encodings-hot-mask", ("encodings",), call("test_gpu_encodings", "test_hot_event_mask", fixture("encodings_golden"), lambda fx: _mod("ebfi_amd.encodings"))),
    ("encodings-stack2cnt", ("encodings",), call("test_gpu_encodings", "test_stack2cnt", fixture("encodings_golden"), lambda fx: _mod("ebfi_amd.encodings"))),
    ("encodings-stack-polarity", ("encodings",), call("test_gpu_encodings", "test_stack_polarity_is_events_to_stack", fixture("golden_dir"), lambda fx: _mod("ebfi_amd.encodings"))),
    ("events-fixtures", ("encodings",), call("test_gpu_events_blur", "test_events_bit_exact_vs_reference_fixtures", fixture("golden_dir"))),
    ("events-degenerate", ("encodings",), call("test_gpu_events_blur", "test_events_degenerate")),
    ("blur-lap-dcp", ("blur",), call("test_gpu_events_blur", "test_frame2lap_frame2dcp_vs_oracle")),
    ("esim-33x65-9", ("esim",), call("test_gpu_esim", "test_device_equals_restatement", 33, 65, 9)),
    ("esim-2x130-2", ("esim",), call("test_gpu_esim", "test_device_equals_restatement", 2, 130, 2)),
    ("esim-chunks-of-3", ("esim",), call("test_gpu_esim", "test_chunking_carries_the_state", 3)),
    ("esim-bgr", ("esim",), call("test_gpu_esim", "test_from_bgr_equals_mono_of_the_restated_gray")),
    ("eventvis-counts", ("eventvis",), call("test_gpu_eventvis", "test_seed_generated_cases_equal_the_host_restatement", "counts72x100")),
    ("eventvis-reals", ("eventvis",), call("test_gpu_eventvis", "test_seed_generated_cases_equal_the_host_restatement", "reals136x200")),
    ("eventvis-fixtures", ("eventvis",), call("test_gpu_eventvis", "test_every_fixture_case_in_all_eight_modes", fixture("eventvis_golden"), lambda fx: list(_mod("test_gpu_eventvis").CASES)[0])),
    ("telemetry-segment-stats", ("telemetry",), call("test_gpu_telemetry", "test_segment_stats_against_the_restatement", fixture("telemetry_case"))),
    ("telemetry-clamped-offsets", ("telemetry",), call("test_gpu_telemetry", "test_offsets_outside_the_buffer_are_clamped")),
    ("telemetry-panels", ("telemetry", "monitor"), call("test_gpu_telemetry", "test_panels_equal_the_reference_compositions")),
    # ---- recurrent.py, gan.py, upsample.py, the optimisers of dp.py
    ("recurrent-lstm-cell", ("recurrent",), call("test_gpu_recurrent", "test_lstm_cell_kernels_against_float64", (2, 16, 33, 4), 1.0)),
    ("recurrent-bilinear-up", ("recurrent",), call("test_gpu_recurrent", "test_bilinear_up_against_float64", (1, 2, 9, 33), 4)),
    ("recurrent-net-lstm", ("recurrent", "unet", "conv"), call("test_gpu_recurrent", "test_whole_net_fp32_against_float64", fixture("recurrent_cases"), "A")),
    ("recurrent-net-gru-x3", ("recurrent", "unet", "conv"), call("test_gpu_recurrent", "test_whole_net_bf16x3_against_float64", fixture("recurrent_cases"), "B")),
    ("gan-bn-lrelu", ("gan",), call("test_gpu_stgan", "test_bn_lrelu_forward_and_backward_within_four_times_torch_float32", (1, 16, 33, 4), 0.0, 1.0)),
    ("gan-linear", ("gan",), call("test_gpu_stgan", "test_linear_layers_within_four_times_torch_float32", 2, 7, 5)),
    ("gan-temporal-bce", ("gan",), call("test_gpu_stgan", "test_temporal_input_and_its_adjoint_and_the_bce_pair")),
    ("gan-odd-maps", ("gan",), call("test_gpu_stgan", "test_odd_maps_against_the_restatement")),
    ("upsample-avgpool2", ("upsample",), call("test_gpu_upsample", "test_avgpool2", (5, 4, 6))),
    ("upsample-bilinear-up2", ("upsample",), call("test_gpu_upsample", "test_bilinear_up2", (2, 5, 7))),
    ("upsample-assemble", ("upsample",), call("test_gpu_upsample", "test_assemble_warps", 64, 96, "fractional")),
    ("upsample-blend", ("upsample",), call("test_gpu_upsample", "test_blend", 32, 32)),
    ("upsample-unet", ("upsample",), call("test_gpu_upsample", "test_unet_forward", "flow", 6, 32, 32)),
    ("upsample-fixture-pair", ("upsample",), call("test_gpu_upsample", "test_fixture_pair")),
    ("optim-native-flat-adam", ("dp",), call("test_gpu_model", "test_native_flat_adam_matches_torch_adam")),
    ("optim-gradient-gather", ("dp",), call("test_gpu_model", "test_native_gradient_gather_packs_like_cat_and_carries_the_guard_flag")),
    ("optim-clip-under-accumulation", ("dp", "engine", "graphstep"), call("test_gpu_gradclip", "test_under_accumulation_the_norm_is_the_windows")),
    # ---- what else allocates (tests/test_poison_host.py: the completeness check): event augmentation, frame io, the loaders
    ("eventaug-augment", ("eventaug",), call("test_gpu_eventaug", "test_augment_kernel_equals_the_restatement", fixture("eventaug_source"), "whole", (True, True), 2 ** 32 + 5, "dense")),
    ("frameio-upload-ragged", ("frameio",), call("test_gpu_frameio", "test_frames_to_planar_is_the_cpu_expression", "ragged_5x7")),
    ("frameio-upload-crop", ("frameio",), call("test_gpu_frameio", "test_frames_to_planar_is_the_cpu_expression", "odd_origin_crop")),
    ("frameio-planar-to-u8", ("frameio",), call("test_gpu_frameio", "test_planar_to_u8_is_the_numpy_expression", (3, 5, 7))),
    ("frameio-period-frames", ("frameio",), call("test_gpu_period_frames", "test_period_to_planar_is_the_cpu_expression", "many_blocks")),
    ("clipdata-device-items", ("clipdata", "frameio", "encodings"), call("test_gpu_clip_loader", "test_device_items_equal_host_items_under_every_augmentation", fixture("clip_synthetic"), "random_crop")),
    # ---- the whole model against the oracle (the bit-for-bit steps are the tests below)
    ("model-train-step-vs-oracle", ("model", "engine", "conv", "fac", "dcn", "fold3d", "loss", "fused", "norm"),
     model_train_step),
]
BY_ID = {c[0]: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------ fixtures
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def four():
    M = _mod("test_gpu_wgrad_multi")
    ops = M._operands(M.ITEMS, 1234)
    return ops, M._dev(ops), [M._reference(op) for op in ops]


@pytest.fixture(scope="module")
def alex_weights(tmp_path_factory):
    return _mod("test_lpips_host").write_weights(tmp_path_factory.mktemp("poisoned_lpips_alex"), seed=0)


@pytest.fixture(scope="module")
def vgg_weights(tmp_path_factory):
    return _mod("lpips_vgg_ref").write_weights(tmp_path_factory.mktemp("poisoned_lpips_vgg"), seed=0)


@pytest.fixture(scope="module")
def vgg_yardstick(vgg_weights):
    """The yardstick of test_gpu_lpips_vgg for the kind "random": per case the inputs and the float64 layer terms, the bar 10 x
    the worst relative layer error of the float32 evaluation over ALL of the kind's cases -- the bar that module computes."""
    L = _mod("test_gpu_lpips_vgg")
    _, _, (ws, bs, heads) = vgg_weights
    cases, worst = {}, 0.0
    for case in L.CASES:
        n, c, h, w, kind = case
        if kind != "random":
            continue
        pred, target = L._pair(n, c, h, w, seed=n * 1000 + h, kind=kind)
        want, want_layers = L.ref_lpips(pred, target, ws, bs, heads)
        _, f32_layers = L.ref_lpips(pred, target, ws, bs, heads, dtype=torch.float32)
        assert torch.all(want_layers > 0)
        worst = max(worst, ((f32_layers.double() - want_layers).abs() / want_layers).max().item())
        cases[case] = (pred, target, want, want_layers)
    assert 0 < L.FACTOR * worst < 1e-2
    return cases, {"random": L.FACTOR * worst}


def _grad_yardstick(ref, factor, kind="random"):
    """The yardstick of the two LPIPS gradient modules for one kind: every case that sets the kind's bar (the dead and the
    flat case are held to it and do not set it), float64 and float32 CPU autograd, bar = factor x the worst float32 error."""
    cases, worst = {}, 0.0
    for case in ref.CASES:
        if case[4] in ("dead", "flat") or ref.kind_of_bar(case[4]) != kind:
            continue
        ws, bs, heads = ref.trunk_of(case)
        pred, target, normalize = ref.make_pair(case)
        go = ref.grad_out_of(case[0])
        want, lpips = ref.ref_grad(pred, target, ws, bs, heads, go, normalize)
        f32, _ = ref.ref_grad(pred, target, ws, bs, heads, go, normalize, dtype=torch.float32)
        assert torch.isfinite(want).all() and torch.isfinite(f32).all()
        errs = [e for e in ref.pair_errors(f32, want) if e is not None]
        assert len(errs) == sum(1 for g in go if g != 0)
        cases[case] = (pred, target, normalize, go, want, lpips)
        worst = max(worst, max(errs))
    assert 0 < factor * worst < 1e-2
    return cases, {kind: factor * worst}


@pytest.fixture(scope="module")
def alex_grad_yardstick():
    return _grad_yardstick(_mod("lpips_alex_grad_ref"), _mod("test_gpu_lpips_alex_grad").FACTOR)


@pytest.fixture(scope="module")
def vgg_grad_yardstick():
    return _grad_yardstick(_mod("lpips_vgg_grad_ref"), _mod("test_gpu_lpips_vgg_grad").FACTOR)


@pytest.fixture(scope="module")
def census_images():
    """As the `images` fixture of test_gpu_census_pair: per shape two predictions, the target and the oracle's two census terms
    with their gradients.  The same draws in the same order, so every shape holds the tensors it holds there."""
    P = _mod("test_gpu_census_pair")
    torch.manual_seed(21)
    out = {}
    for (H, W) in P.SHAPES:
        xa, xb, y = torch.rand(P.B, P.C, H, W), torch.rand(P.B, P.C, H, W), torch.rand(P.B, P.C, H, W)
        refs = []
        for x in (xa, xb):
            xr = x.clone().requires_grad_()
            l = P.loss_ref.census_loss(xr, y)
            l.backward()
            refs.append((l.item(), xr.grad))
        out[(H, W)] = (xa, xb, y, refs)
    return out


def _npz(name):
    import numpy as np
    return np.load(os.path.join(HERE, "golden", name))


@pytest.fixture(scope="module")
def bc_golden():
    return _npz("bc_small.npz")


@pytest.fixture(scope="module")
def iwe_golden():
    return _npz("iwe_small.npz")


@pytest.fixture(scope="module")
def encodings_golden():
    return _npz("encodings_small.npz")


@pytest.fixture(scope="module")
def eventvis_golden():
    return _npz("eventvis_small.npz")


@pytest.fixture(scope="module")
def telemetry_case():
    """The "exact" case of test_gpu_telemetry's parametrised fixture (limits on values the data holds exactly, specials in)."""
    T = _mod("test_gpu_telemetry")
    limits = T.EXACT_LIMITS
    x = T._data(limits, 12, specials=True)
    return limits, x, T.TR.segment_stats_ref(x, T.OFFSETS, limits), T.TR.sum_bounds(x, T.OFFSETS)


@pytest.fixture(scope="module")
def recurrent_cases():
    """The `cases` fixture of test_gpu_recurrent for the two nets the table runs (convlstm and convgru)."""
    import numpy as np
    T = _mod("test_gpu_recurrent")
    seeds = np.load(os.path.join(HERE, "golden", "unet_small.npz"))["seeds"]
    out = {}
    for i, case in enumerate(T.R.CASES):
        if case not in ("A", "B"):
            continue
        seed = int(seeds[i])
        xs, cots = T.R.make_inputs(seed + 1000, case)
        state = T.R.fill_state(seed, case)
        out[case] = (seed, xs, cots, T.R.run(case, state, xs, cots), T.R.run(case, state, xs, cots, dtype=torch.float32))
    return out


@pytest.fixture(scope="module")
def eventaug_source():
    import numpy as np
    T = _mod("test_gpu_eventaug")
    a = np.random.RandomState(7).poisson(0.6, size=(2, T.TB, T.H, T.W)).astype(np.float32)
    dev = torch.from_numpy(a).cuda().transpose(0, 1)
    return dev, a.transpose(1, 0, 2, 3)


@pytest.fixture(scope="module")
def clip_synthetic(tmp_path_factory):
    from ebfi_amd import clipdata
    return clipdata.write_synthetic_clip(str(tmp_path_factory.mktemp("poisoned_clip") / "clip.npz"), num_imgs=17, H=32, W=32,
                                         events_per_frame=300, seed=3)


@pytest.fixture(scope="module")
def model_fix(golden_dir):
    import ast
    import numpy as np
    z = np.load(os.path.join(golden_dir, "model_small.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd.")}
    return z, sd, ast.literal_eval(str(z["cfg"]))


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("cid", [c[0] for c in CASES])
def test_reference_check_on_poisoned_allocations(cid, request):
    _, _, run = BY_ID[cid]
    _drop_cached_workspaces()
    try:
        with poisoned_allocations() as seen:
            run(request.getfixturevalue)
            torch.cuda.synchronize()
    finally:
        _drop_cached_workspaces()                     # (no later test inherits a workspace that was handed out poisoned)
    print("%s: %d poisoned device allocations, %d bytes" % (cid, seen.allocations, seen.bytes))
    assert seen.allocations > 0, "%s made no device allocation through the patched allocators: the patch missed the wrapper" % cid


def _parting(names, sizes, a, b):
    """Which parameters' packed gradients differ between two runs (the report of test_training_step_is_bit_reproducible)."""
    bad, off = [], 0
    for n, sz in zip(names, sizes):
        x, y = a[off:off + sz], b[off:off + sz]
        if not torch.equal(x.view(torch.int32), y.view(torch.int32)):
            bad.append((n, ((x - y).abs().max() / x.abs().max().clamp_min(1e-30)).item()))
        off += sz
    same = [n for n in names if n not in {b[0] for b in bad}]
    return "%d of %d parameter gradients differ (worst %.1e); DIFFERENT: %s; IDENTICAL: %s" % (
        len(bad), len(names), max([b[1] for b in bad] + [0.0]), " ".join(b[0] for b in bad), " ".join(same))


def _same_steps(make, steps):
    """`make()` -> (engine, batches); the same steps poisoned and not, from the same seed: losses, every step's packed gradient
    and the final parameters bit for bit."""
    import contextlib
    runs = []
    for poisoned in (False, True):
        with (poisoned_allocations() if poisoned else contextlib.nullcontext()) as seen:
            eng, batches = make()
            names = [n for n, p in eng.model.named_parameters() if p.requires_grad]
            sizes = [p.numel() for p in eng.bucket.params]
            losses, grads = [], []
            for k in range(steps):
                losses.append(eng.train_step(*batches[k]).item())
                grads.append(eng.bucket.flat.detach().clone())
            torch.cuda.synchronize()
            runs.append((losses, grads, eng.optimizer.flat.detach().clone(), eng))
        if poisoned:
            assert seen.allocations > 0
            print("poisoned steps: %d device allocations, %d bytes" % (seen.allocations, seen.bytes))
    (la, ga, pa, _), (lb, gb, pb, eng) = runs
    for k in range(steps):
        assert torch.equal(ga[k].view(torch.int32), gb[k].view(torch.int32)), "step %d, poisoned against clean: %s" % (k, _parting(names, sizes, ga[k], gb[k]))
    assert la == lb, (la, lb)
    assert torch.equal(pa.view(torch.int32), pb.view(torch.int32))
    return eng


def test_training_steps_do_not_read_what_the_allocator_left():
    """Engine(dict(step=3), seed=21, graph=True, precision="bf16x3"), four steps on 3 x 48 x 80 batches (nothing a power of two):
    the eager calibration steps, the capture and one replay, all with poisoned buffers (a fill inside the capture is a memset
    node of the graph), against the same four steps on clean allocations."""
    from ebfi_amd.engine import Engine, synthetic_batch

    def make():
        eng = Engine(dict(step=3), device="cuda", seed=21, graph=True, precision="bf16x3")
        return eng, [synthetic_batch(3, 48, 80, device="cuda", seed=500 + k) for k in range(4)]

    eng = _same_steps(make, 4)
    assert eng.book is not None and eng.book.skipped_steps() == 0 and len(eng._graphs) == 1


def test_exposure_step_does_not_read_what_the_allocator_left():
    """One stage-1 step of the exposure engine (the ExposureDecision head, the duty / MSE loss), poisoned against clean."""
    X = _mod("test_gpu_exposure")

    def make():
        eng = X._engine("RGBLap", "bf16x3", lr=1e-4)
        return eng, [[v.cuda() for v in X._batch(3, 32, 40, seed=31)]]

    eng = _same_steps(make, 1)
    assert eng.iteration == 1 and eng.bucket.views_intact()


def test_inference_scores_do_not_read_what_the_allocator_left(alex_weights):
    """frame_metrics and the LPIPS score of one prediction, as infer_ours.infer_clip calls them, poisoned against clean."""
    import contextlib
    from ebfi_amd.lpips import load_lpips
    from ebfi_amd.metrics import frame_metrics
    lin_path, backbone_path, _ = alex_weights
    g = torch.Generator().manual_seed(77)
    target = torch.rand(5, 3, 49, 130, generator=g).cuda()
    pred = (target + 0.08 * torch.randn(5, 3, 49, 130, generator=g).cuda()).clamp(0, 1)
    out = []
    for poisoned in (False, True):
        _drop_cached_workspaces()
        with (poisoned_allocations() if poisoned else contextlib.nullcontext()) as seen:
            lpips = load_lpips("alex", lin_path, backbone_path, device="cuda")
            scores = list(frame_metrics(pred, target)) + [lpips(pred, target, normalize=True)]
            torch.cuda.synchronize()
            out.append([s.detach().clone() for s in scores])
        _drop_cached_workspaces()
    assert seen.allocations > 0
    for name, a, b in zip(("psnr", "ssim", "mse", "lpips"), *out):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, a, b)
