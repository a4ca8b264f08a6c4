"""Float64 statements of the convolution routes of ebfi_amd.conv (csrc/conv2d.hip and its three .inc.hpp files), the error bound
the GPU tests hold them to, the case table, and the prediction of the profiler labels each case must produce.  No tests here:
tests/test_conv_routes_host.py checks this file on the CPU, tests/test_gpu_conv_routes.py uses it on the device.

STATEMENTS.  conv64 is torch's CPU convolution in float64; the gradients are torch.nn.grad.conv2d_input / conv2d_weight in
float64.  Every compute mode is a statement about the OPERAND IMAGES the kernels multiply (accumulation is fp32 on the device and
float64 here, so only accumulation error separates the two):
    fp32     conv64(a, b)
    bf16     conv64(bf(a), bf(b))                                  bf(v) = v.bfloat16()
    bf16x3   conv64(al, bh) + conv64(ah, bl) + conv64(ah, bh)      ah = bf(a), al = bf(a - ah)   (csrc/conv2d.hip:806-808)
    f16      conv64(q(a, sa), q(b, sb))                            q(v, s) = (v * s).half() / s, s the slot's power of two
with (a, b) = (x, w) forward, (g * act', w) for the data gradient and (x, g * act') for the weight gradient.  act' comes from the
DEVICE's saved output (a LeakyReLU output within rounding of zero may carry either sign: not what these tests are about) and
g * act' is formed in fp32, as the kernels form it; the bias gradient is the float64 sum of g * act'.

YARDSTICK AND BOUND.  The same statement with torch's CPU fp32 convolutions (S32); per result
    e32 = max|S32 - S64|,  eK = max|device - S64|,  eK <= FACTOR * e32 + 4 * 2^-24 * max|S64|
(the convention of tests/test_gpu_edhead.py; FACTOR = 8 unless FACTORS names the kernel).

ROUTES.  `route(case)` restates the dispatch rules of ebfi_amd/conv.py (ConvBiasAct.backward, _site_backward) and of the launch
code (launch_fwd_bf16, ebfi_conv2d_backward_weight_ex, thin_wgrad_plan, launch_wgrad_shift, ebfi_conv2d_backward_weight_f16g_ex)
for the shapes of the table: the labels N.prof_collect() must show, the arithmetic of each result, and the template instance.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

NONE, LEAKY, SIGMOID = 0, 1, 2
FACTOR = 8.0
# results of kernels that need more than the project's factor: (label, result) -> factor (twice the largest measured eK/e32,
# rounded up to a power of two; the measured ratios are in the docstring of tests/test_gpu_conv_routes.py)
FACTORS = {
    # conv_wgrad_shift<.., THIN_OUT=false, ..> takes the bias gradient from the matrix product itself: an extra A row of ones
    # (csrc/conv2d_shift.inc.hpp:36, MROWS) meets the split images of g * act', so every term enters as hi + lo -- 16 bits, 2^-18
    # relative each -- where torch's pairwise fp32 sum keeps 24.  Over 65536 pixels that is sqrt(N) * 2^-18 = 1e-3 of a term:
    # 10 .. 26 times e32 measured (two draws of the inputs): 2 * 25.75 -> 64.
    ("conv_wgrad_shift/in", "gb"): 64.0,
}
ULPS = 4.0 * 2.0 ** -24
F16_MIN_NORMAL = 2.0 ** -14
# launches every weight gradient / forward brings along: not part of a case's asserted profile
HELPERS = ("conv_wgrad_reduce_f32", "conv_wgrad_reduce_tall", "conv_pack_w_bf16")

Case = collections.namedtuple("Case", "id sect why mode shape act slope bias subset mis layout gpre bank")


def C(id, sect, why, mode, shape, act=NONE, slope=0.01, bias=True, subset="xwb", mis="", layout="", gpre=False, bank=False):
    """shape = (B, Cin, H, W, Cout, k, stride, pad); subset: which of x / w / b require a gradient; mis: which of x / g (the
    gradient handed to backward) sit at data_ptr() % 16 == 4; layout: "slice" (x = a channel slice), "sum" (y.sum().backward())"""
    return Case(id, sect, why, mode, tuple(shape), act, slope, bias, subset, mis, layout, gpre, bank)


def out_hw(shape):
    B, Cin, H, W, Cout, k, s, p = shape
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------------------------------------------ the cases
S9 = (2, 20, 9, 37)             # ragged against every tile: 9 rows (tiles of 4 / 8), 37 columns (tiles of 26..32 / 64), B = 2
BIG_IN = (1, 4, 128, 512, 64, 3, 1, 1)      # the first-layer configuration at the thin / shift plans' minimum of 65536 pixels
# MT = 2 of conv_fwd_bf16x3_db / the wave-specialised form need tiles * ceil(rows / 64) > 128 with rows > 32 (launch_fwd_bf16:
# `few`); tiles = B * ceil(H / TYB) * ceil(W / TX), TYB = 8, TX = 64: B = 17 samples of 9 x 65..68 are 17 * 2 * 2 = 68 tiles, and
# 65..128 rows two blocks: 136 pairs
MT2 = (17, 72, 9)
ACTN = {NONE: "none", LEAKY: "leaky", SIGMOID: "sigmoid"}


def _cases():
    t = []
    # ---- a. gradient subsets through ConvBiasAct
    for cid, shape, act, slope, why in [
        ("k3_leaky_le32", (2, 8, 9, 37, 12, 3, 1, 1), LEAKY, 0.01, "conv_fwd_f32<3,1,1,CK,TR=true,leaky>: Cin <= 32 grid branch"),
        ("k3_relu_gt32", (2, 40, 9, 37, 12, 3, 1, 1), LEAKY, 0.0, "conv_fwd_f32<3,1,2,CK,TR=true,leaky>, slope 0: Cin > 32 grid branch"),
        ("k3_sigmoid_gt32", (1, 40, 5, 70, 3, 3, 1, 1), SIGMOID, 0.0, "conv_fwd_f32<3,1,2,CK,TR=true,sigmoid>"),
        ("k1_leaky_le32", (2, 8, 9, 37, 12, 1, 1, 0), LEAKY, 0.01, "conv_fwd_f32<1,1,1,CK,TR=true,leaky>"),
        ("k1_sigmoid_gt32", (2, 40, 9, 37, 12, 1, 1, 0), SIGMOID, 0.0, "conv_fwd_f32<1,1,2,CK,TR=true,sigmoid>"),
        ("k7_leaky_le32", (1, 6, 9, 37, 5, 7, 1, 3), LEAKY, 0.01, "conv_fwd_f32<7,1,1,2,TR=true,leaky>"),
        ("k7_sigmoid_gt32", (1, 40, 9, 20, 4, 7, 1, 3), SIGMOID, 0.0, "conv_fwd_f32<7,1,2,2,TR=true,sigmoid>"),
        ("k3s2_leaky", (2, 12, 9, 37, 10, 3, 2, 1), LEAKY, 0.01, "stride 2: host-side mask, zero insertion, conv_fwd_f32<3,1,.,TR=true,none>"),
    ]:
        t.append(C("a_x_fp32_" + cid, "a", why, "fp32", shape, act, slope, subset="x"))
    for cid, shape, act, mis, why in [
        ("k3_leaky_v4_mt1", (2, 16, 9, 36, 12, 3, 1, 1), LEAKY, "", "conv_fwd_bf16x3_db<3,1,leaky,4>"),
        ("k3_sigmoid_v4_mt1", (2, 16, 9, 36, 12, 3, 1, 1), SIGMOID, "", "conv_fwd_bf16x3_db<3,1,sigmoid,4>"),
        ("k3_sigmoid_v1_ragged", (2, 16, 9, 37, 12, 3, 1, 1), SIGMOID, "", "conv_fwd_bf16x3_db<3,1,sigmoid,1>: VEC=1 by ragged W"),
        ("k3_leaky_v1_pad", (2, 16, 9, 38, 12, 3, 1, 0), LEAKY, "", "conv_fwd_bf16x3_db<3,1,leaky,1>: VEC=1 by g.pad != KS/2 (Wo % 4 == 0)"),
        ("k3_leaky_v1_misaligned", (2, 16, 9, 36, 12, 3, 1, 1), LEAKY, "g", "conv_fwd_bf16x3_db<3,1,leaky,1>: VEC=1 by a misaligned gradient"),
        ("k1_leaky_v4_mt1", (2, 16, 9, 36, 12, 1, 1, 0), LEAKY, "", "conv_fwd_bf16x3_db<1,1,leaky,4>"),
        ("k1_sigmoid_v1_mt1", (2, 16, 9, 37, 12, 1, 1, 0), SIGMOID, "", "conv_fwd_bf16x3_db<1,1,sigmoid,1>"),
        ("k3_leaky_v4_mt2", MT2 + (68, 8, 3, 1, 1), LEAKY, "", "conv_fwd_bf16x3_db<3,2,leaky,4>"),
        ("k3_sigmoid_v1_mt2", MT2 + (65, 8, 3, 1, 1), SIGMOID, "", "conv_fwd_bf16x3_db<3,2,sigmoid,1>"),
        ("k3_sigmoid_v4_mt2", MT2 + (68, 8, 3, 1, 1), SIGMOID, "", "conv_fwd_bf16x3_db<3,2,sigmoid,4>"),
        ("k3_leaky_v1_mt2", MT2 + (65, 8, 3, 1, 1), LEAKY, "", "conv_fwd_bf16x3_db<3,2,leaky,1>"),
        ("k1_sigmoid_v4_mt2", MT2 + (68, 8, 1, 1, 0), SIGMOID, "", "conv_fwd_bf16x3_db<1,2,sigmoid,4>"),
        ("k1_leaky_v1_mt2", MT2 + (65, 8, 1, 1, 0), LEAKY, "", "conv_fwd_bf16x3_db<1,2,leaky,1>"),
        ("k7_leaky_falls_to_f32", (1, 6, 9, 37, 5, 7, 1, 3), LEAKY, "", "7x7 with a folded derivative: conv_fwd_f32<7,1,1,2,TR=true,leaky> by rule"),
    ]:
        t.append(C("a_x_x3_" + cid, "a", why, "bf16x3", shape, act, subset="x", mis=mis))
    for act in (NONE, LEAKY, SIGMOID):
        a = ACTN[act]
        t.append(C("a_wb_fp32_k3_" + a, "a", "conv_wgrad_f32<3,1,WTXO,%s>, gpre_out == nullptr" % a, "fp32", S9 + (12, 3, 1, 1), act, subset="wb"))
        t.append(C("a_wb_x3_k3_" + a, "a", "conv_wgrad_x3<3,32,%s,WXT,0>, gpre_out == nullptr" % a, "bf16x3", S9 + (12, 3, 1, 1), act, subset="wb"))
        t.append(C("a_wb_x3ws_k3_" + a, "a", "conv_wgrad_x3_ws<%s>, gpre_out == nullptr" % a, "bf16x3", (2, 64, 9, 37, 12, 3, 1, 1), act, subset="wb"))
        t.append(C("a_wb_bf16_k3_" + a, "a", "conv_wgrad_bf16<3,%s>" % a, "bf16", S9 + (12, 3, 1, 1), act, subset="wb"))
        t.append(C("a_wb_x3_shift_in_" + a, "a", "conv_wgrad_shift<3,4,false,4,ALIGNED=true,GPOUT=false>, %s: the first layer of training" % a,
                   "bf16x3", BIG_IN, act, subset="wb"))
    t += [
        C("a_wb_fp32_k1_none", "a", "conv_wgrad_f32<1,1,0,none>, gpre_out == nullptr", "fp32", S9 + (12, 1, 1, 0), NONE, subset="wb"),
        C("a_wb_fp32_k7_sigmoid", "a", "conv_wgrad_f32<7,1,0,sigmoid>, gpre_out == nullptr", "fp32", (1, 6, 9, 37, 5, 7, 1, 3), SIGMOID, subset="wb"),
        C("a_wb_fp32_k3s2_sigmoid", "a", "conv_wgrad_f32<3,2,0,sigmoid>, gpre_out == nullptr", "fp32", (2, 12, 9, 37, 10, 3, 2, 1), SIGMOID, subset="wb"),
        C("a_wb_fp32_k7s2_leaky", "a", "conv_wgrad_f32<7,2,0,leaky>, gpre_out == nullptr", "fp32", (1, 6, 10, 37, 8, 7, 2, 3), LEAKY, subset="wb"),
        C("a_wb_x3_k1_leaky", "a", "conv_wgrad_x3<1,0,leaky,WXT,0>, gpre_out == nullptr", "bf16x3", S9 + (12, 1, 1, 0), LEAKY, subset="wb"),
        C("a_wb_x3_k7_sigmoid", "a", "conv_wgrad_x3<7,32,sigmoid,WXT,0>, gpre_out == nullptr", "bf16x3", (1, 6, 9, 37, 5, 7, 1, 3), SIGMOID, subset="wb"),
        C("a_wb_x3_k3_small_wg_leaky", "a", "conv_wgrad_x3<3,32,leaky,256,32>: the 32-channel workgroup, gpre_out == nullptr", "bf16x3",
          (2, 32, 9, 37, 12, 3, 1, 1), LEAKY, subset="wb"),
        C("a_wb_bf16_k1_leaky", "a", "conv_wgrad_bf16<1,leaky>", "bf16", S9 + (12, 1, 1, 0), LEAKY, subset="wb"),
        C("a_wb_fp32_thin_in_leaky", "a", "conv_wgrad_thin<1,4,1,false>, gp == nullptr", "fp32", BIG_IN, LEAKY, subset="wb"),
        C("a_wb_fp32_thin_in_none", "a", "conv_wgrad_thin<1,4,1,false>, no activation, gp == nullptr", "fp32", BIG_IN, NONE, subset="wb"),
        C("a_wb_fp32_thin_ins2_sigmoid", "a", "conv_wgrad_thin<2,4,1,false>, gp == nullptr", "fp32", (2, 4, 256, 512, 16, 3, 2, 1), SIGMOID, subset="wb"),
        C("a_wb_x3_shift_in_dword_leaky", "a", "conv_wgrad_shift<3,4,false,4,ALIGNED=false,GPOUT=false>: rows that are not whole quads",
          "bf16x3", (1, 4, 129, 510, 64, 3, 1, 1), LEAKY, subset="wb"),
        C("a_b_fp32_k3_leaky", "a", "bias only: conv_wgrad_f32<3,1,WTXO,leaky> runs for the bias column, gpre_out == nullptr", "fp32",
          S9 + (12, 3, 1, 1), LEAKY, subset="b"),
        C("a_b_x3ws_k3_sigmoid", "a", "bias only: conv_wgrad_x3_ws<sigmoid>, gpre_out == nullptr", "bf16x3", (2, 64, 9, 37, 12, 3, 1, 1), SIGMOID, subset="b"),
    ]
    # ---- b. paddings other than k // 2, all three gradients
    for mode in ("fp32", "bf16x3", "bf16"):
        for k, s, p in [(3, 1, 0), (3, 1, 2), (3, 2, 0), (3, 2, 2), (7, 1, 1), (7, 1, 5), (7, 1, 6), (7, 2, 0), (7, 2, 2), (1, 1, 0),
                        (1, 1, 1), (3, 1, 3), (7, 1, 7), (3, 2, 3)]:
            if mode == "bf16" and not (s == 1 and k in (1, 3)):
                continue                                  # (every other layer runs the fp32 kernels in that mode: covered by "fp32")
            if mode == "bf16x3" and s == 2:
                continue                                  # (stride 2 runs the fp32 kernels in that mode; 7x7 pad 0 / 2 / 3 by parity or
                                                          #  zero insertion is tests/test_gpu_conv.py's stride-2 7x7 test)
            shape = (2, 10, 9, 37, 12, k, s, p) if k < 7 else (1, 6, 12, 37, 5, 7, s, p)
            why = "pad %d of a %dx%d stride-%d layer%s: the dword / masked-halo paths at g.pad != KS/2" % (
                p, k, k, s, " (pad == k: backward drops the outer ring, conv._crop_rings)" if p == k else "")
            t.append(C("b_%s_k%ds%dp%d" % (mode, k, s, p), "b", why, mode, shape, LEAKY))
    t.append(C("b_bank_k3s1p3", "b", "a bank site at pad == k: _site_backward drops the outer ring for the packed split-precision data gradient",
               "bf16x3", (2, 10, 9, 37, 12, 3, 1, 3), LEAKY, bank=True))
    # ---- c. pointers and layouts
    WS = MT2 + (68, 128, 3, 1, 1)          # 136 (tile, output-channel block) pairs forward and (tile, input-channel block) pairs backward
    t += [
        C("c_x3_ws_aligned", "c", "control: conv_fwd_bf16x3_ws<0> forward and data gradient on aligned operands", "bf16x3", WS, LEAKY),
        C("c_x3_misaligned_x", "c", "conv_fwd_bf16x3_db<3,2,none,1> forward instead of _ws: aligned16(x) of vec4 (conv2d.hip launch_fwd_bf16)",
          "bf16x3", WS, LEAKY, mis="x"),
        C("c_x3_misaligned_g", "c", "conv_fwd_bf16x3_db<3,2,none,1> data gradient instead of _ws: aligned16(grad_output) of vec4", "bf16x3", WS,
          NONE, mis="g"),
        C("c_fp32_thin_misaligned_x", "c", "conv_wgrad_f32<3,1,WTXO,leaky> instead of conv_wgrad_thin/in: thin_wgrad_plan's aligned16(x)", "fp32",
          BIG_IN, LEAKY, subset="wb", mis="x"),
        C("c_fp32_thin_misaligned_g", "c", "conv_wgrad_f32<3,1,WTXO,leaky> instead of conv_wgrad_thin/in: thin_wgrad_plan's aligned16(go)", "fp32",
          BIG_IN, LEAKY, mis="g"),
        C("c_x3_shift_misaligned_g", "c", "conv_wgrad_shift<3,4,false,4,ALIGNED=false,GPOUT=false>: `al` of launch_wgrad_shift", "bf16x3", BIG_IN,
          LEAKY, subset="wb", mis="g"),
        C("c_x3_shift_misaligned_g_gpout", "c", "conv_wgrad_shift<3,4,false,4,ALIGNED=false,GPOUT=true>", "bf16x3", BIG_IN, LEAKY, mis="g"),
        C("c_bank_c64_misaligned_x", "c", "conv_wgrad_f16_ws<leaky> instead of conv_wgrad_f16_tr: tr_ok's aligned16(input)", "bf16x3",
          (2, 64, 9, 36, 64, 3, 1, 1), LEAKY, subset="wb", mis="x", bank=True),
        C("c_bank_c64_misaligned_g", "c", "conv_wgrad_f16_ws<none> instead of conv_wgrad_f16_tr: tr_ok's aligned16(grad_output)", "bf16x3",
          (2, 64, 9, 36, 64, 3, 1, 1), NONE, subset="wb", mis="g", bank=True),
        C("c_bank_c48_misaligned_x", "c", "conv_wgrad_x3<3,32,leaky,WXT,0> instead of the fp16 kernels: al16 of _site_backward (ragged Cin)",
          "bf16x3", (2, 48, 9, 36, 32, 3, 1, 1), LEAKY, subset="wb", mis="x", bank=True),
        C("c_bank_c64_x_misaligned_g", "c", "conv_fwd_bf16x3_db<3,1,none,1> data gradient instead of conv_fwd_f16_ws: the quad-staging fp16 "
          "kernel refuses an unaligned input", "bf16x3", (2, 64, 9, 36, 64, 3, 1, 1), NONE, subset="x", mis="g", bank=True),
        C("c_fp32_channel_slice", "c", "x[:, 1:]: the .contiguous() of ConvBiasAct.forward", "fp32", S9 + (12, 3, 1, 1), LEAKY, layout="slice"),
        C("c_x3_sum_backward", "c", "y.sum().backward(): a stride-0 gradient through .contiguous()", "bf16x3", S9 + (12, 3, 1, 1), LEAKY, layout="sum"),
    ]
    # ---- d. grad_preact=True
    t += [C("d_%s_grad_preact" % m, "d", "grad_preact=True: backward as for no activation, no output saved", m, S9 + (12, 3, 1, 1), LEAKY, gpre=True)
          for m in ("fp32", "bf16x3")]
    # ---- e. bank site with the scale book
    for act in (LEAKY, SIGMOID):
        a = ACTN[act]
        t.append(C("e_wb_f16_tr_" + a, "e", "conv_wgrad_f16_tr<%s>, grad_preact_out == nullptr" % a, "bf16x3", (2, 64, 9, 36, 64, 3, 1, 1), act,
                   subset="wb", bank=True))
        t.append(C("e_wb_f16_ws_" + a, "e", "conv_wgrad_f16_ws<%s>, grad_preact_out == nullptr" % a, "bf16x3", (2, 64, 9, 37, 64, 3, 1, 1), act,
                   subset="wb", bank=True))
    t += [
        C("e_x_f16_none", "e", "conv_fwd_f16_ws on the transposed fp16 image, source parameters frozen", "bf16x3", (2, 64, 9, 36, 64, 3, 1, 1), NONE,
          subset="x", bank=True),
        C("e_x_x3_leaky_folded", "e", "packed ebfi_conv2d_backward_data_bf16x3 with the folded derivative: conv_fwd_bf16x3_db<3,1,leaky,4>", "bf16x3",
          (2, 64, 9, 36, 64, 3, 1, 1), LEAKY, subset="x", bank=True),
    ]
    ids = [c.id for c in t]
    assert len(set(ids)) == len(ids)
    return t


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------------------------ the routes
def _cdiv(a, b):
    return -(-a // b)


def _x3_kernel(role, B, rows, Ho, Wo, w_in, pad_same, aligned, k, dact):
    """launch_fwd_bf16 (csrc/conv2d.hip) with x3 != 0: rows = output channels of the product run, Ho x Wo its output map, w_in the
    row length of its input -> (label, MT, VEC)"""
    tiles = B * _cdiv(Ho, 8) * _cdiv(Wo, 64)                       # TYB = 8, TX = 64
    few = tiles * _cdiv(rows, 64) <= 128
    mt = 1 if (rows <= 32 or few) else 2
    vec4 = w_in % 4 == 0 and pad_same and aligned
    ws = k == 3 and mt == 2 and vec4 and dact == NONE
    return ("conv_fwd_bf16x3_ws/" if ws else "conv_fwd_bf16x3_db/") + role, mt, (4 if vec4 and dact != NONE else 1)


def _thin_kind(shape, x_al, g_al):
    """thin_wgrad_plan (csrc/conv2d_thin.inc.hpp:309-332); y and gp are fresh allocations, aligned"""
    B, Cin, H, W, Cout, k, s, p = shape
    Ho, Wo = out_hw(shape)
    if Wo % 4 or W % 4 or B * Ho * Wo < 65536 or not (x_al and g_al):
        return None
    tpr = Wo // 4
    if tpr > 256 or 256 % tpr:
        return None
    if k == 3 and s == 1 and p == 1:
        return "out" if (Cout <= 4 and Cin >= 16) else ("in" if (Cin <= 4 and Cout >= 16) else None)
    return "ins2" if (k == 3 and s == 2 and p == 1 and Cin <= 4 and Cout >= 16) else None


def _shift_kind(shape):
    """shift_wgrad_geometry (csrc/conv2d_shift.inc.hpp:398-410)"""
    B, Cin, H, W, Cout, k, s, p = shape
    Ho, Wo = out_hw(shape)
    if s != 1 or B * Ho * Wo < 65536:
        return None
    if k == 3 and p == 1:
        return "out" if (Cout in (1, 3) and Cin == 64) else ("in" if (Cin == 4 and Cout == 64) else None)
    return "out7" if (k == 7 and p == 0 and Cout == 3 and Cin == 16) else None


def _wgrad_x3(shape, act, gp_out, inst):
    B, Cin, H, W, Cout, k, s, p = shape
    inst.update(wgrad_act=act, gp_out=gp_out)
    return "conv_wgrad_x3_ws" if (k == 3 and Cin % 64 == 0) else "conv_wgrad_x3"


def route(c):
    """(labels, arith, inst): the conv* profiler labels of forward + backward without HELPERS; the arithmetic ("fp32" | "bf16" |
    "bf16x3" | "f16") of y, gx and gw; the instance parameters the dispatch fixes (dgrad_da / dgrad_vec / dgrad_mt / f32_dgrad_rows /
    wgrad_act / gp_out / shift_aligned)."""
    B, Cin, H, W, Cout, k, s, p = c.shape
    Ho, Wo = out_hw(c.shape)
    x_al = "x" not in c.mis                       # (a channel slice goes through .contiguous(): a fresh, aligned tensor)
    g_al = "g" not in c.mis                       # (a stride-0 gradient likewise)
    need_x = "x" in c.subset
    need_w = "w" in c.subset or ("b" in c.subset and c.bias)
    act = NONE if c.gpre else c.act               # what backward sees
    labels, ar, inst = set(), {}, {}
    mode = c.mode
    assert not (k == 3 and s == 1 and p == 1 and Cout <= 3 and 16 <= Cin <= 64 and Cin % 16 == 0 and B * H * W >= 65536 and mode == "bf16x3"), \
        "the tap-row thin forward is tests/test_gpu_conv.py's: no case here selects it"
    if c.bank:
        assert mode == "bf16x3" and k == 3 and s == 1 and B * Ho * Wo < 65536
        lab, _, _ = _x3_kernel("fwd", B, Cout, Ho, Wo, W, p == 1, x_al, k, NONE)
        labels.add(lab)
        ar["y"] = "bf16x3"
        al16 = x_al and g_al
        f16 = p == 1                                  # the fp16 backward kernels: 3x3 same-padded layers
        f16_w = f16 and (Cin % 64 == 0 or (Cin >= 32 and W % 4 == 0 and al16))
        f16_x = f16 and W % 4 == 0 and Cin >= 48
        gp_side = need_w and need_x and act != NONE
        gp16 = gp_side and f16_w and f16_x and al16 and Cout % 16 == 0
        if need_w:
            if f16_w:
                tr_ok = W % 4 == 0 and x_al and g_al
                labels.add("conv_wgrad_f16_tr/f32" if tr_ok else "conv_wgrad_f16_ws")
                inst.update(wgrad_act=act, gp_out=gp_side)
                ar["gw"] = "f16"
            else:
                labels.add(_wgrad_x3(c.shape, act, gp_side, inst))
                ar["gw"] = "bf16x3"
        if need_x:
            src_al = True if gp_side else g_al
            dact = NONE if gp_side else act
            if gp16:
                labels.add("conv_fwd_f16_ws/img_f32")
                ar["gx"] = "f16"
            elif f16_x and src_al and dact == NONE:
                labels.add("conv_fwd_f16_ws/f32_f32")
                ar["gx"] = "f16"
            else:
                ring = max(p - (k - 1), 0)            # pad == k: conv._crop_rings hands the kernel fresh tensors at pad k-1
                lab, mt, vec = _x3_kernel("dgrad", B, Cin, H, W, Wo - 2 * ring, (k - 1 - (p - ring)) == k // 2, src_al or ring > 0, k, dact)
                labels.add(lab)
                inst.update(dgrad_da=dact, dgrad_vec=vec, dgrad_mt=mt)
                ar["gx"] = "bf16x3"
        return labels, ar, inst
    # ---- ConvBiasAct.forward
    bf16 = mode == "bf16" and k in (1, 3) and s == 1
    if bf16:
        labels.add("conv_fwd_bf16/fwd")
        ar["y"] = "bf16"
    elif mode == "bf16x3" and s == 1 and (k in (1, 3) or (k == 7 and Cout <= 16)):
        labels.add("conv7_x3/fwd" if k == 7 else _x3_kernel("fwd", B, Cout, Ho, Wo, W, p == k // 2, x_al, k, NONE)[0])
        ar["y"] = "bf16x3"
    else:
        labels.add("conv_fwd_f32/fwd")
        ar["y"] = "fp32"
    # ---- ConvBiasAct.backward
    gp_side = need_w and need_x and act != NONE and not bf16          # grad * act' leaves the weight-gradient kernel
    if need_w:
        x3w = mode == "bf16x3" and s == 1
        shift = _shift_kind(c.shape) if x3w else None
        thin = _thin_kind(c.shape, x_al, g_al)
        if shift:
            labels.add("conv_wgrad_shift/" + shift)
            thick_al = (x_al if shift != "in" else g_al)
            inst.update(wgrad_act=act, gp_out=gp_side, shift_aligned=(W if shift != "in" else Wo) % 4 == 0 and thick_al)
            ar["gw"] = "bf16x3"
        elif thin:
            labels.add("conv_wgrad_thin/" + thin)
            inst.update(wgrad_act=act, gp_out=gp_side)
            ar["gw"] = "fp32"
        elif bf16:
            labels.add("conv_wgrad_bf16")
            inst.update(wgrad_act=act, gp_out=False)
            ar["gw"] = "bf16"
        elif x3w:
            labels.add(_wgrad_x3(c.shape, act, gp_side, inst))
            ar["gw"] = "bf16x3"
        else:
            labels.add("conv_wgrad_f32")
            inst.update(wgrad_act=act, gp_out=gp_side)
            ar["gw"] = "fp32"
    if need_x:
        ring = max(p - (k - 1), 0)                    # pad == k: conv._crop_rings hands the kernels fresh tensors at pad k-1
        src_al = True if (gp_side or (ring and s == 1)) else g_al
        dact = NONE if gp_side else act
        wo_d, p_d = (Wo - 2 * ring, k - 1) if (ring and s == 1) else (Wo, p)
        if bf16:
            labels.add("conv_fwd_bf16/dgrad")
            ar["gx"] = "bf16"
        elif mode == "bf16x3" and s == 1 and (k in (1, 3) or (k == 7 and Cin <= 16)) and (k != 7 or gp_side or act == NONE):
            if k == 7:
                labels.add("conv7_thin_dgrad" if (Cout == 3 and Cin == 16 and B * H * W >= 65536) else "conv7_x3/dgrad")
            else:
                lab, mt, vec = _x3_kernel("dgrad", B, Cin, H, W, wo_d, (k - 1 - p_d) == k // 2, src_al, k, dact)
                labels.add(lab)
                inst.update(dgrad_da=dact, dgrad_vec=vec, dgrad_mt=mt)
            ar["gx"] = "bf16x3"
        elif s == 2 and k == 7 and mode == "bf16x3" and Cin <= 16:
            labels.add("conv7_x3/dgrad_s2" if p == 3 else "conv7_x3/dgrad")
            ar["gx"] = "bf16x3"
        else:
            labels.add("conv_fwd_f32/dgrad")
            inst.update(dgrad_da=(dact if s == 1 else NONE), f32_dgrad_rows="le32" if Cin <= 32 else "gt32")
            ar["gx"] = "fp32"
    return labels, ar, inst


# what the table must reach: (name, predicate over (case, labels, inst)) -- closed by tests/test_conv_routes_host.py
def _req_f32_dgrad(da, slope0=None, k=None, rows=None, s=None):
    def pred(c, labels, inst):
        return ("conv_fwd_f32/dgrad" in labels and c.subset == "x" and c.mode == "fp32" and (da is None or inst.get("dgrad_da") == da) and
                (slope0 is None or (c.slope == 0.0) == slope0) and (k is None or c.shape[5] == k) and
                (rows is None or inst.get("f32_dgrad_rows") == rows) and (s is None or c.shape[6] == s))
    return pred


def _req_x3_dgrad(da, vec, mt, k):
    return lambda c, labels, inst: ("conv_fwd_bf16x3_db/dgrad" in labels and c.subset == "x" and inst.get("dgrad_da") == da and
                                    inst.get("dgrad_vec") == vec and inst.get("dgrad_mt") == mt and c.shape[5] == k)


def _req_wb(label, act=None, k=None, s=None, **kw):
    def pred(c, labels, inst):
        return (label in labels and c.subset in ("wb", "b") and inst.get("gp_out") is False and (act is None or inst.get("wgrad_act") == act) and
                (k is None or c.shape[5] == k) and (s is None or c.shape[6] == s) and all(inst.get(a) == v for a, v in kw.items()))
    return pred


def _required():
    r = [("a: x only, fp32, leaky slope 0.01", _req_f32_dgrad(LEAKY, slope0=False)), ("a: x only, fp32, leaky slope 0", _req_f32_dgrad(LEAKY, slope0=True)),
         ("a: x only, fp32, sigmoid", _req_f32_dgrad(SIGMOID)), ("a: x only, fp32, stride-2 3x3", _req_f32_dgrad(None, k=3, s=2))]
    r += [("a: x only, fp32, k=%d" % k, _req_f32_dgrad(None, k=k, s=1)) for k in (1, 3, 7)]
    r += [("a: x only, fp32, Cin %s grid branch" % b, _req_f32_dgrad(None, rows=b)) for b in ("le32", "gt32")]
    for da in (LEAKY, SIGMOID):
        for vec in (4, 1):
            for mt in (1, 2):
                r.append(("a: x only, bf16x3, _db/dgrad DA=%s VEC=%d MT=%d" % (ACTN[da], vec, mt),
                          lambda c, l, i, da=da, vec=vec, mt=mt: any(_req_x3_dgrad(da, vec, mt, k)(c, l, i) for k in (1, 3))))
    r += [("a: x only, bf16x3, k=%d" % k, lambda c, l, i, k=k: any(_req_x3_dgrad(da, v, m, k)(c, l, i) for da in (LEAKY, SIGMOID) for v in (1, 4) for m in (1, 2)))
          for k in (1, 3)]
    r += [("a: VEC=1 by ragged W", lambda c, l, i: c.sect == "a" and i.get("dgrad_vec") == 1 and i.get("dgrad_da") and out_hw(c.shape)[1] % 4 != 0),
          ("a: VEC=1 by pad != k//2", lambda c, l, i: c.sect == "a" and i.get("dgrad_vec") == 1 and i.get("dgrad_da") and out_hw(c.shape)[1] % 4 == 0 and
           c.shape[7] != c.shape[5] // 2 and not c.mis),
          ("a: VEC=1 by a misaligned pointer", lambda c, l, i: c.sect == "a" and i.get("dgrad_vec") == 1 and i.get("dgrad_da") and
           out_hw(c.shape)[1] % 4 == 0 and c.shape[7] == c.shape[5] // 2 and "g" in c.mis),
          ("a: x only, bf16x3, k=7 with an activation -> fp32 kernel", lambda c, l, i: c.mode == "bf16x3" and c.shape[5] == 7 and c.subset == "x" and
           c.act != NONE and "conv_fwd_f32/dgrad" in l)]
    for act in (NONE, LEAKY, SIGMOID):
        r.append(("a: w and b only, act %s" % ACTN[act], lambda c, l, i, act=act: c.subset == "wb" and i.get("wgrad_act") == act and i.get("gp_out") is False))
    r += [("a: w and b only, conv_wgrad_f32 k=%d s=%d" % (k, s), _req_wb("conv_wgrad_f32", k=k, s=s)) for k, s in ((1, 1), (3, 1), (7, 1), (3, 2), (7, 2))]
    r += [("a: w and b only, " + lab, _req_wb(lab)) for lab in ("conv_wgrad_x3", "conv_wgrad_x3_ws", "conv_wgrad_bf16", "conv_wgrad_thin/in",
                                                                 "conv_wgrad_thin/ins2")]
    r += [("a: w and b only, conv_wgrad_shift/in aligned", _req_wb("conv_wgrad_shift/in", shift_aligned=True)),
          ("a: w and b only, conv_wgrad_shift/in dword", _req_wb("conv_wgrad_shift/in", shift_aligned=False)),
          ("a: b only", lambda c, l, i: c.subset == "b")]
    for mode in ("fp32", "bf16x3", "bf16"):
        pads = [(3, 1, 0), (3, 1, 2), (1, 1, 0)] + ([(3, 2, 0), (3, 2, 2), (7, 2, 0), (7, 2, 2)] if mode == "fp32" else []) + \
               ([(7, 1, 1), (7, 1, 5), (7, 1, 6)] if mode != "bf16" else [])
        pads += [(1, 1, 1), (3, 1, 3)] + ([(7, 1, 7)] if mode != "bf16" else [])
        for k, s, p in pads:
            r.append(("b: %s k=%d s=%d pad=%d, all three gradients" % (mode, k, s, p),
                      lambda c, l, i, m=mode, ksp=(k, s, p): c.sect == "b" and c.mode == m and c.shape[5:] == ksp and c.subset == "xwb"))
    r += [("c: _db instead of _ws by misaligned x", lambda c, l, i: "x" in c.mis and "conv_fwd_bf16x3_db/fwd" in l and
           route(c._replace(mis=""))[0] >= {"conv_fwd_bf16x3_ws/fwd"}),
          ("c: _db instead of _ws by a misaligned gradient", lambda c, l, i: "g" in c.mis and "conv_fwd_bf16x3_db/dgrad" in l and
           route(c._replace(mis=""))[0] >= {"conv_fwd_bf16x3_ws/dgrad"}),
          ("c: conv_wgrad_f32 instead of conv_wgrad_thin", lambda c, l, i: c.mis and "conv_wgrad_f32" in l and
           any(x.startswith("conv_wgrad_thin") for x in route(c._replace(mis=""))[0])),
          ("c: the dword shift instance by a misaligned pointer", lambda c, l, i: c.mis and "conv_wgrad_shift/in" in l and i.get("shift_aligned") is False and
           route(c._replace(mis=""))[2].get("shift_aligned") is True),
          ("c: bank, conv_wgrad_f16_ws instead of _tr (Cin % 64 == 0)", lambda c, l, i: c.bank and c.mis and "conv_wgrad_f16_ws" in l and
           "conv_wgrad_f16_tr/f32" in route(c._replace(mis=""))[0]),
          ("c: bank, split-precision weight gradient for Cin = 48", lambda c, l, i: c.bank and c.mis and c.shape[1] == 48 and "conv_wgrad_x3" in l and
           "conv_wgrad_f16_tr/f32" in route(c._replace(mis=""))[0]),
          ("c: channel-sliced x", lambda c, l, i: c.layout == "slice"), ("c: y.sum().backward()", lambda c, l, i: c.layout == "sum")]
    r += [("d: grad_preact=True, " + m, lambda c, l, i, m=m: c.gpre and c.mode == m and c.act == LEAKY) for m in ("fp32", "bf16x3")]
    for act in (LEAKY, SIGMOID):
        for lab in ("conv_wgrad_f16_tr/f32", "conv_wgrad_f16_ws"):
            r.append(("e: bank, w and b only, %s %s, no gp" % (lab, ACTN[act]),
                      lambda c, l, i, act=act, lab=lab: c.bank and not c.mis and c.subset == "wb" and lab in l and i.get("wgrad_act") == act and i.get("gp_out") is False))
    r += [("e: bank, x only, act none -> conv_fwd_f16_ws/f32_f32", lambda c, l, i: c.bank and not c.mis and c.subset == "x" and c.act == NONE and
           "conv_fwd_f16_ws/f32_f32" in l),
          ("e: bank, x only, act leaky -> packed split-precision data gradient, folded", lambda c, l, i: c.bank and c.subset == "x" and
           "conv_fwd_bf16x3_db/dgrad" in l and i.get("dgrad_da") == LEAKY)]
    return r


REQUIRED = _required()


# ------------------------------------------------------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(x, w, b, g) of case `cid` on the CPU in fp32; shared, never modified.  Gaussian, scaled as in tests/test_gpu_conv.py; the
    fp16 (bank) cases draw magnitudes uniformly from [1/64, 1] with a random sign, so that no scaled operand is an fp16 subnormal."""
    c = BY_ID[cid]
    B, Cin, H, W, Cout, k, s, p = c.shape
    Ho, Wo = out_hw(c.shape)
    gen = torch.Generator().manual_seed(7000 + CASES.index(c))
    if c.bank:
        u = lambda *shape: ((1 / 64 + (1 - 1 / 64) * torch.rand(*shape, generator=gen)) *
                            (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()
        x, w, g = u(B, Cin, H, W), u(Cout, Cin, k, k) / (Cin * k * k) ** 0.5, u(B, Cout, Ho, Wo)
    else:
        x = torch.randn(B, Cin, H, W, generator=gen)
        w = torch.randn(Cout, Cin, k, k, generator=gen) / (Cin * k * k) ** 0.5
        g = torch.randn(B, Cout, Ho, Wo, generator=gen)
    b = torch.randn(Cout, generator=gen) * 0.1 if c.bias else None
    if c.layout == "sum":
        g = torch.ones_like(g)
    return x, w, b, g


def scale_law(amax):
    """The pinned slot law of csrc/scale_law.hpp: the power of two that puts amax into [2, 4), its exponent at most 120."""
    amax = float(amax)
    if not (amax > 0 and math.isfinite(amax)):
        return 1.0
    return 2.0 ** min(2 - math.frexp(amax)[1], 120)


def first_use_scales(c, x, w, g):
    """{x, g, w}: what a fresh ScaleBook calibrates from -- the input, the gradient AS IT ARRIVES (before act'), the weight"""
    return {"x": scale_law(x.abs().max()), "g": scale_law(g.abs().max()), "w": scale_law(w.abs().max())}


# ------------------------------------------------------------------------------------------------------------------ the statements
def act_fwd(v, act, slope):
    return F.leaky_relu(v, slope) if act == LEAKY else (torch.sigmoid(v) if act == SIGMOID else v)


def grad_preact(g, y, act, slope):
    """g * act'(y) in fp32, as the kernels form it (act_grad of csrc/conv2d.hip: through the OUTPUT y)"""
    if act == LEAKY:
        return g * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    if act == SIGMOID:
        return g * (y * (1 - y))
    return g


def bf(v):
    return v.float().bfloat16().float()


def split(v):
    h = bf(v)
    return h, bf(v.float() - h)


def q16(v, s):
    return ((v.float() * s).half().double() / s)


def images(a, b, arith, sa=None, sb=None):
    """the pairs of operand images whose products the mode accumulates, in the kernels' order"""
    if arith == "fp32":
        return [(a, b)]
    if arith == "bf16":
        return [(bf(a), bf(b))]
    if arith == "bf16x3":
        (ah, al), (bh, bl) = split(a), split(b)
        return [(al, bh), (ah, bl), (ah, bh)]
    if arith == "f16":
        return [(q16(a, sa), q16(b, sb))]
    raise ValueError(arith)


def evaluate(op, pairs, dt):
    acc = None
    for a, b in pairs:
        t = op(a.to(dt), b.to(dt))
        acc = t if acc is None else acc + t
    return acc


def ops(c):
    """the three bilinear maps of the case: forward, data gradient (g', w), weight gradient (x, g')"""
    B, Cin, H, W, Cout, k, s, p = c.shape
    return (lambda X, Wt: F.conv2d(X, Wt, None, s, p),
            lambda G, Wt: torch.nn.grad.conv2d_input((B, Cin, H, W), Wt, G, stride=s, padding=p),
            lambda X, G: torch.nn.grad.conv2d_weight(X, (Cout, Cin, k, k), G, stride=s, padding=p))


NAMES = ("y", "gx", "gw", "gb")


def wanted(c):
    """which results the case compares"""
    return [n for n, on in zip(NAMES, (True, "x" in c.subset, "w" in c.subset, "b" in c.subset and c.bias)) if on]


def act_deriv(y, act, slope):
    """act'(y) in fp32 through the output y (act_grad_c of csrc/conv2d.hip)"""
    if act == LEAKY:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    return y * (1 - y) if act == SIGMOID else torch.ones_like(y)


def folded(c, inst=None):
    """the case's data gradient is a split-precision kernel that multiplies by act' while it stages (no grad * act' tensor)"""
    inst = route(c)[2] if inst is None else inst
    return route(c)[1].get("gx") == "bf16x3" and inst.get("dgrad_da", NONE) != NONE


def statement(c, y_dev, dt, scales=None, arith=None, tweak=None, gp_tweak=None, fused_lo=False):
    """{y, gx, gw, gb} of the case in dtype dt (None where the case does not ask for it).  y_dev: the output whose activation
    derivative backward uses (the device's own; None: the statement's own y in fp32).  fused_lo: see below.  tweak(name, op, pairs, dt) / gp_tweak(gp, g, y):
    where the host test plants a defect (in place of `evaluate` / on g * act')."""
    x, w, b, g = inputs(c.id)
    arith = arith or route(c)[1]
    scales = scales or {}
    fwd, dgrad, wgrad = ops(c)
    ev = lambda name, op, pairs: tweak(name, op, pairs, dt) if tweak else evaluate(op, pairs, dt)
    pre = ev("y", fwd, images(x, w, arith["y"]))
    if b is not None:
        pre = pre + b.to(dt).view(1, -1, 1, 1)
    res = {"y": act_fwd(pre, c.act, c.slope), "gx": None, "gw": None, "gb": None}
    y = res["y"].float() if y_dev is None else y_dev
    assert not (fused_lo and not folded(c))
    gp = g if c.gpre else grad_preact(g, y, c.act, c.slope)
    if gp_tweak:
        gp = gp_tweak(gp, g, y)
    if "gx" in wanted(c):
        pairs = images(gp, w, arith["gx"], scales.get("g"), scales.get("w"))
        if fused_lo:
            # the staging code of a folded derivative reads `v *= act'; hi = bf16(v); lo = bf16(v - hi)` (conv2d.hip commit()):
            # under the compiler's default contraction `v - hi` may become fma(g, act', -hi), i.e. lo is taken from the
            # UNROUNDED product.  Both are the split of g * act'; the GPU test admits either.
            hi = bf(gp)
            lo = bf((g.double() * act_deriv(y, c.act, c.slope).double() - hi.double()).float())
            wh, wl = split(w)
            pairs = [(lo, wh), (hi, wl), (hi, wh)]
        res["gx"] = ev("gx", dgrad, pairs)
    if "gw" in wanted(c):
        res["gw"] = ev("gw", wgrad, images(x, gp, arith["gw"], scales.get("x"), scales.get("g")))
    if "gb" in wanted(c):
        res["gb"] = gp.to(dt).sum(dim=(0, 2, 3))
    return res


def factor_for(labels, name):
    """FACTOR, or the factor FACTORS gives result `name` of a kernel among `labels`"""
    return max([FACTOR] + [f for (l, n), f in FACTORS.items() if l in labels and n == name])


def check_bound(tag, got, s64, s32, names, labels=(), out=print):
    """[(name, e32, eK, bound)] of the results outside eK <= factor * e32 + 4 * 2^-24 * max|S64|; prints every figure"""
    bad = []
    for n in names:
        a, b32, k = s64[n].double(), s32[n].double(), got[n].double()
        assert k.shape == a.shape, (tag, n, k.shape, a.shape)
        e32, ek, scale = (b32 - a).abs().max().item(), (k - a).abs().max().item(), a.abs().max().item()
        bound = factor_for(labels, n) * e32 + ULPS * scale
        out("%-36s %-3s e32 %.3e  eK %.3e  eK/e32 %8.2f  bound %.3e  max|S64| %.3e"
            % (tag, n, e32, ek, ek / e32 if e32 > 0 else (float("inf") if ek > 0 else 0.0), bound, scale))
        if not ek <= bound:                            # (a NaN fails too)
            bad.append((n, e32, ek, bound))
    return bad
