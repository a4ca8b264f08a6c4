/*
 * ebfi_hip.h -- C ABI of libebfi_hip.so: the MI355X (gfx950) kernels behind the EBFI-BE
 * frame-synthesis hot path.  Plain pointers and sizes only; every pointer marked "device" is a
 * HIP device address, `stream` is a hipStream_t (NULL = the legacy default stream).
 *
 * Conventions
 *   - every entry point returns EBFI_OK (0) or a negative ebfi_status; it never throws and never
 *     allocates device memory.  ebfi_last_error() returns a thread-local description of the last
 *     failure on the calling thread.
 *   - launches are asynchronous on `stream`; the library keeps no global mutable state besides the
 *     optional profiler (ebfi_prof_*), so distinct streams/threads may call concurrently.
 *   - dtype: every floating tensor of a call is fp32 in memory (EBFI_F32), like the reference's ops; the
 *     other ebfi_dtype values select the matrix-core OPERAND precision of the convolution kernels
 *     (fp32 accumulation always).  Shapes/strides are in ELEMENTS, NCHW order of the LOGICAL dims
 *     (a channels-last tensor is passed with its real strides).
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   ebfi_fac_forward / ebfi_fac_backward
 *       pybind module `kernelconv2d_cuda`: forward / backward
 *       models/FAC/kernelconv2d/KernelConv2D_cuda.cpp:10-61, kernels KernelConv2D_kernel.cu:25-204
 *   ebfi_dcn_forward / ebfi_dcn_backward
 *       pybind module `_ext`: dcn_v2_forward / dcn_v2_backward
 *       models/DCNv2/src/dcn_v2.h:9-92, src/vision.cpp:4-9, src/cuda/dcn_v2_cuda.cu:20-216,
 *       src/cuda/dcn_v2_im2col_cuda.cu:125-402
 *   ebfi_dcn_pooling_forward / ebfi_dcn_pooling_backward
 *       pybind module `_ext`: dcn_v2_psroi_pooling_forward / dcn_v2_psroi_pooling_backward
 *       models/DCNv2/src/vision.cpp:7-8, src/cuda/dcn_v2_psroi_pooling_cuda.cu:58-419
 *   ebfi_conv2d_*               nn.Conv2d + activation inside ConvLayer (models/model_misc/submodules.py:159-200)
 *   ebfi_scale_residual_cat_*   exposure/time-scaled residual + concat of ResidualControl (model_singleframe.py:124-134)
 *   ebfi_prodmean_*             AdaptiveAvgPool2d(1) of a product of two maps (ExposureDecision, model_singleframe.py:66-68)
 *   ebfi_se_gate_*              SEGating (+ residual + ReLU / LeakyReLU) of the detail branch (models/model_misc/resnet_3D.py:89-141)
 *   ebfi_ed_head_*              GroupNorm x2 -> pooled product -> sigmoid -> scaled concat of ExposureDecision (model_singleframe.py:66-72)
 *   ebfi_groupnorm_*            nn.GroupNorm of ExposureDecision (models/Ours/model_singleframe.py:36,66-67)
 *   ebfi_census_*               Ternary census loss (loss/restore.py:108-145)
 *   ebfi_gauss5_*               GaussianConv of the Laplacian-pyramid loss (loss/restore.py:149-163)
 *   ebfi_laploss_*              whole Laplacian-pyramid L1 term of a step as one difference pyramid (loss/restore.py:166-213)
 *   ebfi_adam_step              optimizer.step() of train_ours.py:276-277 over the flat parameter buffer
 *   ebfi_optim_step             the same for every optimiser the config may name: torch.optim.Adam / AdamW / SGD (train_ours.py:770-771)
 *   ebfi_grad_norm              the norm and coefficient of torch.nn.utils.clip_grad_norm_ over the flat gradient, left on the device
 *   ebfi_optim_step_ex          ebfi_optim_step with that coefficient and an exponential moving average of the weights in the same
 *                               launch (no counterpart in the reference, which trains without either)
 *   ebfi_grad_gather            gradient bucket packing of DistributedDataParallel (train_ours.py:754) as one launch
 *   ebfi_gather_sum             weight re-layouts of the depth-2 Conv3d / ConvTranspose3d (models/model_misc/resnet_3D.py)
 *   ebfi_events_to_stack        dataloader/encodings.py:307-350 (events_to_stack)
 *   ebfi_events_to_grid / ebfi_interpolate_to_image / ebfi_hot_event_mask / ebfi_stack_to_cnt / ebfi_polarity_mask
 *                               the rest of dataloader/encodings.py: voxel grids, images, stacks, channels, masks (:8-74, :102-150,
 *                               :204-304, :353-430) as ordered fp32 sums
 *   ebfi_iwe_*                  myutils/iwe.py (get_interpolation, interpolate, deblur_events, compute_pol_iwe) and loss/flow.py
 *                               (EventWarping with its gradient into the flow, AveragedIWE) as ordered fp32 sums
 *   ebfi_bc_* / ebfi_sobel_*    loss/reconstruction.py (BrightnessConstancy: generative model, temporal consistency, total variation)
 *                               and myutils/gradients.py (Sobel), each with its gradients; the grid_sample adjoint as an ordered fp32 sum
 *   ebfi_frame2lap / _frame2dcp myutils/utils.py:34-49 / :15-31
 *   ebfi_frames_u8_to_planar    GetFrames of the real-data reader (dataloader/h5dataset_realdata.py:178-189) + AugmentData's crop / flips
 *   ebfi_planar_to_u8           the uint8 image cast of the evaluation loop (infer_ours.py:135)
 *   ebfi_period_frames_u8       GetFrames of the synthetic-blur reader (dataloader/h5dataset.py:296-311): sharp frames + exposure mean
 *   ebfi_event_augment / ebfi_event_hot_pixels
 *                               AugmentData's crop, flips, add_noise and add_hot_pixels on the event stack
 *                               (dataloader/h5dataset.py:368-463), with a counter-based integer noise law
 *   ebfi_event_cnt_image        event_visualisation.plot_event_cnt of the evaluation loop (infer_ours.py:139-142,
 *                               myutils/vis_events/matplotlib_plot_events.py:127-251)
 *   ebfi_segment_stats          per-layer weight / gradient moments and histograms of the training monitor (no counterpart in the
 *                               reference: its TensorBoard log holds scalars and images only)
 *   ebfi_esim_*                 esim_py.EventSimulator of the dataset step (generate_dataset/syn_gopro.py:77-81,115-116)
 *   ebfi_avgpool2_forward / ebfi_bilinear_up2_forward / ebfi_flow_max_magnitude / ebfi_slomo_*
 *                               the Vid2E adaptive upsampler (generate_dataset/upsampling/utils/{upsampler,model}.py)
 *   ebfi_image_metrics          psnr_loss / ssim_loss / nn.MSELoss of the evaluation loop (loss/restore.py:43-92, infer_ours.py:120-128)
 *   ebfi_lpips_*                perceptual_loss(net='alex') of the evaluation loop (loss/restore.py:10-40, LPIPS v0.1) and, as
 *                               ebfi_lpips_alex_forward_train / _backward, of the training loss (train_ours.py:765)
 *   ebfi_lpips_vgg*             perceptual_loss(net='vgg'), likewise
 *   ebfi_charbonnier_*          CharbonnierLoss of the validation loop (loss/restore.py:95-105, train_ours.py:588)
 *   ebfi_duty_head_*            tail of ExposureDecision.forward + nn.MSELoss of stage 1 (model_singleframe.py:75-76,
 *                               train_ours_exposuredecision.py:250-252)
 *   ebfi_bn_lrelu_* / ebfi_stgan_temporal_* / ebfi_linear_* / ebfi_bce_logits_pair / ebfi_adamax_step
 *                               Adversarial(gan_type='STGAN') of the training loss dictionary (train_ours.py:767,
 *                               loss/adversarial.py, loss/discriminator.py:208-263): BatchNorm2d + LeakyReLU in training mode,
 *                               the temporal input, F.binary_cross_entropy_with_logits and torch.optim.Adamax
 */
#ifndef EBFI_HIP_H
#define EBFI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (bumped whenever an entry point is added or changed; the Python binding refuses any other value):
 *   3  round 2/3 additions (ebfi_ed_head_*, ebfi_laploss_*, ebfi_se_gate_*, ebfi_adam_step, ebfi_pack_table_bf16,
 *      ebfi_conv2d_packed_x3, the fused KernelConv -> FAC forward, ...)
 *   4  ebfi_se_gate_forward takes a workspace (ebfi_se_gate_workspace)
 *   5  (round 4) the never-implemented EBFI_BF16 storage value left ebfi_dtype; fp16 filter storage and the fused-gradient
 *      entry points of the KernelConv -> FAC training path (ebfi_fac_forward_p16 / _backward_p16, ebfi_conv2d_packed_*_c16,
 *      ebfi_conv2d_backward_weight_f16c*, ebfi_to_c16, ebfi_scale_residual_cat_*_c16)
 *   6  fp16-operand FORWARD: ebfi_pack_table_f16 writes forward weight images too; ebfi_conv2d_packed_f16_c16 takes the
 *      planar-fp16 output form (the 128 -> 1600 KernelConv of the training step)
 *   7  EpiExtra masks from fp16 images: ebfi_conv2d_packed_f16_c16 takes mask_is_c16 (the LeakyReLU derivative read from the
 *      sign of the c16 image instead of an fp32 tensor)
 *   8  ebfi_conv2d_backward_weight_f16g_ex: the weight gradient writes grad * act'(y) as a c16 image for the data gradient
 *   9  (round 5) ebfi_grad_gather (gradient packing + overflow flag in the wire buffer); ebfi_adam_step_guarded takes the
 *      all-reduced flag; ebfi_fac_*_p16 take the unpadded input (replicate padding inside); ebfi_pad2d_backward;
 *      ebfi_conv2d_packed_x3_rc / ebfi_scale_residual_cat_backward_c16a (ResidualControl's tail in the convolution's epilogue)
 *  10  ebfi_conv2d_thin_forward (3x3 layers with <= 3 output channels: taps on the matrix row axis)
 *  11  ebfi_scalar_conv_forward / _backward (ResidualControl's scalar-conditioned channel scales: a bank of 1x1 convolutions on
 *      [B,K,1,1] inputs in one launch each way); ebfi_kernelconv_fac_fused_f16 (the fused KernelConv -> FAC kernel of inference
 *      on fp16 operands)
 *  12  ebfi_se_gate_forward_ps / _backward_ps (the squeeze-excite gate of an up-convolution stage reading the transposed
 *      convolution's output through the pixel shuffle)
 *  13  ebfi_conv2d_packed_x3_shuffled / ebfi_conv2d_packed_f16_shuffled (convolutions storing through PixelShuffle(2) / its inverse)
 *  14  ebfi_to_c16_cat2 (the fp16 image of a two-part channel concatenation without the concatenated tensor); later, as a pure
 *      addition under the same number, ebfi_image_metrics_workspace / ebfi_image_metrics (evaluation PSNR / SSIM / MSE): no
 *      existing entry point changed, so a caller built against an earlier 14 header still calls every function it knows with
 *      the right arguments, and the binding's version check has nothing new to refuse; later still, as another pure addition
 *      under 14, ebfi_lpips_params_bytes / _pack_params / _workspace / _alex (evaluation LPIPS, AlexNet v0.1); and, again as a
 *      pure addition under 14, ebfi_charbonnier_workspace / _forward / _backward (the validation loop's Charbonnier loss); and
 *      ebfi_duty_head_workspace / _forward / _backward (the duty head and MSE loss of the stage-1 pre-training), likewise; and
 *      ebfi_frames_u8_to_planar / ebfi_planar_to_u8 (the frame upload and download of an inference run on recorded clips); and
 *      ebfi_event_cnt_image_workspace / ebfi_event_cnt_image (the event-count images of the evaluation loop), likewise; and
 *      ebfi_period_frames_u8 (the sharp frames and the exposure mean of a training period from its stored bytes), likewise; and
 *      ebfi_esim_loop_bound / _init / _count / _emit (the event simulator of the synthetic-dataset step), likewise; and
 *      ebfi_avgpool2_forward / ebfi_bilinear_up2_forward / ebfi_flow_max_magnitude / ebfi_slomo_assemble / _blend / _frame_u8
 *      (the frame-upsampling step), likewise -- with them ebfi_conv2d_forward accepts ksize 5 at stride 1, which it refused; and
 *      ebfi_lpips_vgg_params_bytes / _pack_params / _workspace / ebfi_lpips_vgg (evaluation LPIPS, VGG-16 v0.1), likewise; and
 *      ebfi_lpips_vgg_train_workspace / ebfi_lpips_vgg_forward_train / ebfi_lpips_vgg_backward (the same as a training loss); and
 *      ebfi_segment_stats_workspace / ebfi_segment_stats (per-layer weight and gradient statistics of the training monitor),
 *      likewise; and ebfi_optim_step (Adam / AdamW with weight decay and AMSGrad, SGD with momentum: the optimiser section of
 *      the training config), likewise; and ebfi_conv2d_backward_weight_f16g_multi_workspace /
 *      ebfi_conv2d_backward_weight_f16g_multi (the pure weight gradients of a training step, deferred and run in one launch) and
 *      ebfi_gather_sum_multi (their fold gathers), likewise; and ebfi_event_augment / ebfi_event_hot_pixels (the device noise
 *      law of the clip loaders), likewise; and ebfi_dcn_pooling_forward / _backward (the deformable PS-ROI pooling of the
 *      DCNv2 package), likewise; and ebfi_grad_norm_workspace / ebfi_grad_norm / ebfi_optim_step_ex (gradient clipping by
 *      total norm and an exponential moving average of the weights around the optimiser step), likewise; and
 *      ebfi_lpips_alex_grad_params_bytes / _pack_grad_params / _train_workspace / _forward_train / _backward (evaluation LPIPS
 *      with the AlexNet trunk as a training loss), likewise; and ebfi_bn_lrelu_workspace / _forward / _backward,
 *      ebfi_stgan_temporal_forward / _backward, ebfi_linear_forward / _backward_data / _backward_weight, ebfi_bce_logits_pair
 *      and ebfi_adamax_step (the STGAN adversarial loss: what
 *      lies between the discriminator's convolutions, and its Adamax), likewise */
#define EBFI_ABI_VERSION 14

typedef enum {
    EBFI_OK = 0,
    EBFI_ERR_ARG = -1,         /* shape / stride / pointer precondition violated */
    EBFI_ERR_LAUNCH = -2,      /* HIP reported a launch error */
    EBFI_ERR_UNSUPPORTED = -3, /* dtype or configuration not implemented */
    EBFI_ERR_WORKSPACE = -4    /* workspace missing or too small */
} ebfi_status;

/* EBFI_F32_BF16MMA: fp32 tensors, operands rounded to bf16 for the matrix cores, fp32 accumulation
 * (accepted by ebfi_conv2d_backward_weight; the forward / data-gradient have *_bf16mma entry points) */
/* (value 1 was a bf16-storage mode that no entry point ever implemented: removed in ABI 5, the number stays unused) */
typedef enum { EBFI_F32 = 0, EBFI_F32_BF16MMA = 2, EBFI_F32_BF16X3MMA = 3 } ebfi_dtype;

int ebfi_abi_version(void);
const char *ebfi_last_error(void);

/* ------------------------------------------------------------------ FAC (filter-adaptive conv)
 * out[b,c,y,x] = sum_{ky,kx} input[b,c,y+ky,x+kx] * kernel[b, c*K*K + ky*K + kx, y, x]
 * input  [B, C, Ho+K-1, Wo+K-1]  (already padded by the caller, KernelConv2D.py:85-87)
 * kernel [B, C*K*K, Ho, Wo],  output [B, C, Ho, Wo].  Any strides; K >= 1.
 * Unlike the reference the outputs need NOT be pre-zeroed: every element is written. */
int ebfi_fac_forward(const void *input, const int64_t input_shape[4], const int64_t input_stride[4],
                     const void *kernel, const int64_t kernel_shape[4], const int64_t kernel_stride[4],
                     int kernel_size,
                     void *output, const int64_t output_shape[4], const int64_t output_stride[4],
                     int dtype, void *stream);

/* grad_input [B,C,Ho+K-1,Wo+K-1], grad_kernel [B,C*K*K,Ho,Wo]; both fully overwritten.
 * Either grad pointer may be NULL to skip it. */
int ebfi_fac_backward(const void *input, const int64_t input_shape[4], const int64_t input_stride[4],
                      const void *kernel, const int64_t kernel_shape[4], const int64_t kernel_stride[4],
                      int kernel_size,
                      const void *grad_output, const int64_t grad_output_stride[4],
                      void *grad_input, const int64_t grad_input_stride[4],
                      void *grad_kernel, const int64_t grad_kernel_stride[4],
                      int dtype, void *stream);

/* Same, with grad_kernel leaving as the gradient of the PRE-activation of the LeakyReLU(kernel_leaky_slope) layer that produced
 * the filters (KernelConv + FAC in Modification, reference models/Ours/model_singleframe.py:161-162): grad_kernel is
 * multiplied by 1 where kernel > 0 and by the slope elsewhere.  kernel_leaky_slope = 1 is ebfi_fac_backward exactly. */
int ebfi_fac_backward_ex(const void *input, const int64_t input_shape[4], const int64_t input_stride[4],
                         const void *kernel, const int64_t kernel_shape[4], const int64_t kernel_stride[4],
                         int kernel_size,
                         const void *grad_output, const int64_t grad_output_stride[4],
                         void *grad_input, const int64_t grad_input_stride[4],
                         void *grad_kernel, const int64_t grad_kernel_stride[4],
                         float kernel_leaky_slope, int dtype, void *stream);

/* ------------------------------------------------------------------ DCNv2 (modulated deformable conv)
 * All tensors contiguous NCHW:
 *   input [B,C,H,W]  weight [Co,C,kh,kw]  bias [Co]
 *   offset [B, dg*2*kh*kw, Ho, Wo]  (channel 2*(i*kw+j) = dy, +1 = dx inside each group block)
 *   mask   [B, dg*kh*kw, Ho, Wo]    output [B,Co,Ho,Wo]
 *   Ho = (H + 2*ph - (dh*(kh-1)+1))/sh + 1, likewise Wo.
 * The column tensor of the reference never exists in memory.
 * ebfi_dcn_forward accepts dtype EBFI_F32 (exact fp32 matrix cores: the kernel the reference's known-answer tests pin)
 * or EBFI_F32_BF16X3MMA (same fp32 tensors; the 64 x C*kh*kw x 64 product runs on the bf16 matrix cores in split
 * precision, ~1e-5 of the exact result).  The backward is fp32 only. */
int ebfi_dcn_forward(const void *input, const void *weight, const void *bias, const void *offset,
                     const void *mask, void *output,
                     int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw,
                     int ph, int pw, int dh, int dw, int deformable_group,
                     int dtype, void *stream);

/* Bytes of scratch ebfi_dcn_backward needs (partial weight-gradient slabs). */
size_t ebfi_dcn_backward_workspace(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw,
                                   int ph, int pw, int dh, int dw, int deformable_group, int dtype);

/* All five gradients are fully (over)written; grad_input is accumulated with float atomics after
 * being zeroed by the library (run-to-run differences in the last bits, like the reference's
 * atomicAdd col2im, dcn_v2_im2col_cuda.cu:249).  Reference quirk kept: grad_input uses pad_h for
 * both axes (dcn_v2_im2col_cuda.cu:368). */
int ebfi_dcn_backward(const void *input, const void *weight, const void *bias, const void *offset,
                      const void *mask, const void *grad_output,
                      void *grad_input, void *grad_offset, void *grad_mask, void *grad_weight,
                      void *grad_bias,
                      int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw,
                      int ph, int pw, int dh, int dw, int deformable_group,
                      void *workspace, size_t workspace_bytes, int dtype, void *stream);

/* ------------------------------------------------------------------ DCNv2 deformable PS-ROI pooling
 * The second op of the reference's DCNv2 package (src/cuda/dcn_v2_psroi_pooling_cuda.cu).  Contiguous fp32:
 *   input [B,C,H,W]   rois [R,5] = (batch index, x1, y1, x2, y2) in image pixels
 *   trans [Rt >= R, 2*nc, part, part] (NULL when no_trans; nc is then 1)
 *   output, count [R, D, P, P]  (D = output_dim, P = pooled_size; count = samples that contributed, as fp32)
 * With G = group_size, spp = sample_per_part, cec = D / nc, every step ONE fp32 operation in this order (no fused
 * multiply-add), for output element (n, d, ph, pw):
 *   sw = round(x1) * scale - 0.5, ew = (round(x2) + 1) * scale - 0.5; sh, eh likewise   (C round(): half away from zero)
 *   rw = max(ew - sw, 0.1f), bw = rw / P, sbw = bw / spp; rh, bh, sbh likewise
 *   part_h = floor(float(ph) / P * part), part_w likewise; cls = d / cec
 *   tx = trans[n, 2*cls, part_h, part_w] * trans_std, ty = trans[n, 2*cls + 1, ..] * trans_std   (0 when no_trans)
 *   w0 = float(pw) * bw + sw, w0 += tx * rw; h0 likewise with ty * rh
 *   gw = clamp(floor(float(pw) * G / P), 0, G - 1), gh likewise; the input channel is c = (d*G + gh)*G + gw
 *   for ih, iw in [0, spp), ih outer: w = w0 + iw * sbw, h = h0 + ih * sbh
 *       skipped when w < -0.5 || w > W - 0.5 || h < -0.5 || h > H - 0.5
 *       else w = fmin(fmax(w, 0), W - 1), h likewise (a NaN coordinate becomes 0 and IS counted), and the sample is
 *       the bilinear interpolation of plane c on the corners floor / ceil with dx = w - floor(w), dy = h - floor(h):
 *       (1-dx)*(1-dy)*U00 + (1-dx)*dy*U01 + dx*(1-dy)*U10 + dx*dy*U11, Uxy = plane at column corner x and row corner y (0 = floor, 1 = ceil),
 *       each product left to right, the four terms added left to right, the samples of a bin added in loop order from 0
 *   output = count ? sum / count : 0
 * Backward, dv = grad_output / count where count > 0: every included sample scatters q00, q01, q10, q11 times dv onto
 * its four corners of grad_input, and adds to the x and y cells (n, cls, part_h, part_w) of grad_trans
 *   (U11*dy + U10*(1-dy) - U01*dy - U00*(1-dy)) * trans_std * dv * rw   and
 *   (U11*dx + U01*(1-dx) - U10*dx - U00*(1-dx)) * trans_std * dv * rh        (0 at an exactly integer coordinate).
 * Two places where the reference reads out of bounds are defined instead:
 *   - channels: the reference asserts C == D and indexes channel (d*G + gh)*G + gw, safe for G == 1 only.  Here
 *     C == D * G * G is required (the reference's rule at G == 1, position-sensitive pooling otherwise), and D % nc == 0.
 *   - batch index: an ROI whose batch index is not an integer value in [0, B) (NaN included) gives output = 0,
 *     count = 0 and no gradient; the reference reads wherever the index points.
 * count may be NULL in the forward.  grad_input [B,C,H,W] is zeroed by the library and accumulated with float atomics
 * (last-bit run-to-run differences, like ebfi_dcn_backward); grad_trans [Rt, 2*nc, part, part] (NULL when no_trans) is
 * zeroed whole -- rows R..Rt-1 stay 0 -- and every cell has ONE writer that sums in a fixed order: bit-reproducible.
 * EBFI_F32 only.  Null pointers, sizes < 1 (R < 0, Rt < R), C != D*G*G, D % nc != 0, P / part / spp < 1 -> EBFI_ERR_ARG;
 * spp > 32, or H * W beyond 2^31 - 1 -> EBFI_ERR_UNSUPPORTED; neither touches the GPU.  R == 0 is a no-op (nothing is written). */
int ebfi_dcn_pooling_forward(const void *input, const void *rois, const void *trans, void *output, void *count,
                             int B, int C, int H, int W, int R, int nc, int no_trans, float spatial_scale,
                             int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part,
                             float trans_std, int dtype, void *stream);

int ebfi_dcn_pooling_backward(const void *grad_output, const void *input, const void *rois, const void *trans,
                              const void *count, void *grad_input, void *grad_trans, int Rt,
                              int B, int C, int H, int W, int R, int nc, int no_trans, float spatial_scale,
                              int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part,
                              float trans_std, int dtype, void *stream);

/* ------------------------------------------------------------------ conv + bias + activation (ConvLayer)
 * What the reference gets from nn.Conv2d + nn.LeakyReLU / nn.Sigmoid inside ConvLayer
 * (models/model_misc/submodules.py:159-200).  Contiguous NCHW fp32.
 *   input [B,Cin,H,W]  weight [Cout,Cin,k,k]  bias [Cout] or NULL  output [B,Cout,Ho,Wo]
 *   k in {1,3}, stride in {1,2}, Ho = (H + 2*pad - k)/stride + 1.  (ebfi_conv2d_forward also: k = 7 at stride 1 and 2, and
 *   k = 5 at stride 1 -- the Super-SloMo U-Net's second stage; the gradients and the bf16 forms refuse k = 5.)
 *   act: 0 none, 1 LeakyReLU(slope), 2 Sigmoid -- fused into the epilogue. */
int ebfi_conv2d_forward(const void *input, const void *weight, const void *bias, void *output,
                        int B, int Cin, int H, int W, int Cout, int ksize, int stride, int pad,
                        int act, float slope, int dtype, void *stream);

/* grad_input = conv^T(grad_output * act'(saved_output)); stride 1, pad = k/2 only.
 * saved_output is the forward OUTPUT (post-activation); may be NULL when act == 0. */
int ebfi_conv2d_backward_data(const void *grad_output, const void *saved_output, const void *weight,
                              void *grad_input, int B, int Cin, int H, int W, int Cout, int ksize,
                              int stride, int pad, int act, float slope, int dtype, void *stream);

size_t ebfi_conv2d_backward_weight_workspace(int B, int Cin, int H, int W, int Cout, int ksize,
                                             int stride, int pad, int dtype);

/* grad_weight [Cout,Cin,k,k] and (if non-NULL) grad_bias [Cout]; fully overwritten; deterministic
 * (per-workgroup partial slabs in `workspace`, fixed-order reduction). */
int ebfi_conv2d_backward_weight(const void *input, const void *grad_output, const void *saved_output,
                                void *grad_weight, void *grad_bias,
                                int B, int Cin, int H, int W, int Cout, int ksize, int stride, int pad,
                                int act, float slope, void *workspace, size_t workspace_bytes,
                                int dtype, void *stream);

/* Same as ebfi_conv2d_backward_weight plus an optional side output
 * grad_preact_out [B,Cout,Ho,Wo] = grad_output * act'(saved_output) (fp32 kernels only; NULL to skip):
 * the caller can then run ebfi_conv2d_backward_data on it with act = 0 and no saved activation. */
int ebfi_conv2d_backward_weight_ex(const void *input, const void *grad_output, const void *saved_output,
                                   void *grad_weight, void *grad_bias, void *grad_preact_out,
                                   int B, int Cin, int H, int W, int Cout, int ksize, int stride, int pad,
                                   int act, float slope, void *workspace, size_t workspace_bytes,
                                   int dtype, void *stream);

/* bf16 matrix-core variants: fp32 tensors in memory, operands rounded to bf16 for v_mfma_f32_32x32x16_bf16,
 * fp32 accumulation (16x the fp32 MFMA rate).  k in {1,3}, stride 1.  `workspace` receives the weight
 * re-packed to bf16 [tap][co][ci16] (ebfi_conv2d_bf16_workspace bytes: room for the hi and lo images of the
 * split-precision variants below). */
size_t ebfi_conv2d_bf16_workspace(int Cin, int Cout, int ksize);
int ebfi_conv2d_forward_bf16mma(const void *input, const void *weight, const void *bias, void *output,
                                int B, int Cin, int H, int W, int Cout, int ksize, int stride, int pad,
                                int act, float slope, void *workspace, size_t workspace_bytes, void *stream);
int ebfi_conv2d_backward_data_bf16mma(const void *grad_output, const void *saved_output, const void *weight,
                                      void *grad_input, int B, int Cin, int H, int W, int Cout, int ksize,
                                      int stride, int pad, int act, float slope,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* Split-precision ("bf16x3") variants: every fp32 operand is carried as hi = bf16(v), lo = bf16(v - hi) and each
 * product is accumulated as hi*hi + hi*lo + lo*hi on the bf16 matrix cores (fp32 accumulation).  Results agree with
 * the exact fp32 kernels to ~1e-5 relative (tests/test_gpu_conv.py), at 3/16 of their matrix-core time.  Same
 * arguments, workspace (ebfi_conv2d_bf16_workspace) and limits as the *_bf16mma functions. */
int ebfi_conv2d_forward_bf16x3(const void *input, const void *weight, const void *bias, void *output,
                               int B, int Cin, int H, int W, int Cout, int ksize, int stride, int pad,
                               int act, float slope, void *workspace, size_t workspace_bytes, void *stream);
int ebfi_conv2d_backward_data_bf16x3(const void *grad_output, const void *saved_output, const void *weight,
                                     void *grad_input, int B, int Cin, int H, int W, int Cout, int ksize,
                                     int stride, int pad, int act, float slope,
                                     void *workspace, size_t workspace_bytes, void *stream);

/* Data gradient of a 7x7 STRIDE-2 convolution with at most 16 input channels (the detail branch's stem,
 * models/model_misc/resnet_3D.py BasicStem folded to 2-D: 6 <- 64 channels) from grad_preact = grad_output * act'(output),
 * split precision, evaluated per output parity class (no zero-inserted gradient tensor).  pad = 3. */
int ebfi_conv2d_backward_data_s2_bf16x3(const void *grad_preact, const void *weight, void *grad_input, int B, int Cin,
                                        int H, int W, int Cout, int ksize, int pad, void *stream);

/* ------------------------------------------------------------------ 5x5 conv + bias + activation
 * The recurrent U-Nets of models/model_misc/unet.py at their default kernel_size = 5: head, stride-2 encoders, up-sampling
 * decoders.  Exact fp32 (v_mfma_f32_32x32x2_f32, fp32 accumulation), contiguous NCHW fp32, no atomics, no allocation and no
 * synchronisation: capturable.  The ebfi_conv2d_* entry points above refuse exactly what they refused before; 5x5 layers
 * with gradients come here.
 *   input [B,Cin,H,W]  weight [Cout,Cin,5,5]  bias [Cout] or NULL  output [B,Cout,Ho,Wo],  Ho = (H + 2*pad - 5)/stride + 1
 *   stride in {1,2}, 0 <= pad <= 4, any B, Cin, Cout, H, W >= 1 with Ho, Wo >= 1, each sample (plus 64 channels) below 2 GiB.
 *   act: 0 none, 1 LeakyReLU(slope) (ReLU = slope 0), 2 Sigmoid.
 * Laws:
 *   forward        output = act(conv(input, weight) + bias), every element written.
 *   backward_data  grad_input = conv^T(grad_output * act'(saved_output)), every element written -- the rows / columns that no
 *                  window reaches when H + 2*pad - 5 is odd at stride 2 as zeros.  saved_output is the forward OUTPUT (act' is
 *                  taken from it: y > 0 ? 1 : slope, or y (1 - y)); NULL iff act == 0.  Stride 1 is the forward kernel on the
 *                  transposed, flipped filter with pad 4 - pad; stride 2 is evaluated per parity class of (y + pad, x + pad) on
 *                  grad_output itself: 3x3, 3x2, 2x3 or 2x2 taps per class, no zero-inserted tensor.
 *   backward_weight  grad_weight [Cout,Cin,5,5] and (if non-NULL) grad_bias [Cout] of the same product, fully overwritten:
 *                  one partial slab per workgroup in `workspace`, summed in a fixed order -- bit-reproducible.  Optional side
 *                  output grad_preact_out [B,Cout,Ho,Wo] = grad_output * act'(saved_output), the very values the kernel
 *                  multiplies: the caller runs backward_data on it with act = 0.
 *   ebfi_conv5x5_backward_weight_workspace: bytes backward_weight needs; 0 for a geometry the entry points refuse.
 * Null pointers, an unknown activation, an activation without saved_output, a non-positive size, an empty output or a
 * sample beyond the 2 GiB reach -> EBFI_ERR_ARG; stride outside {1,2} or pad outside 0..4 -> EBFI_ERR_UNSUPPORTED; a missing
 * or short workspace -> EBFI_ERR_WORKSPACE; none touches the GPU.  B == 0 is a no-op, except that backward_weight zero-fills
 * grad_weight / grad_bias. */
int ebfi_conv5x5_forward(const void *input, const void *weight, const void *bias, void *output,
                         int B, int Cin, int H, int W, int Cout, int stride, int pad,
                         int act, float slope, void *stream);
int ebfi_conv5x5_backward_data(const void *grad_output, const void *saved_output, const void *weight, void *grad_input,
                               int B, int Cin, int H, int W, int Cout, int stride, int pad,
                               int act, float slope, void *stream);
size_t ebfi_conv5x5_backward_weight_workspace(int B, int Cin, int H, int W, int Cout, int stride, int pad);
int ebfi_conv5x5_backward_weight(const void *input, const void *grad_output, const void *saved_output,
                                 void *grad_weight, void *grad_bias, void *grad_preact_out,
                                 int B, int Cin, int H, int W, int Cout, int stride, int pad,
                                 int act, float slope, void *workspace, size_t workspace_bytes, void *stream);

/* Weights packed ahead of the call.  ebfi_conv2d_forward_bf16x3 / ebfi_conv2d_backward_data_bf16x3 re-pack `weight` into
 * `workspace` on every call; when `weight` is NULL they take `workspace` as ALREADY holding the packed images
 * ([hi | lo], bf16 [tap][M][K16]: forward M = Cout, K = Cin; data gradient `transposed`: M = Cin, K = Cout, taps flipped;
 * ebfi_conv2d_packed_bytes bytes) -- weights change once per optimiser step, not once per launch.
 * ebfi_conv2d_pack_bf16x3 packs one weight; ebfi_pack_table_bf16 packs ANY number of weights in one launch from a host-built
 * table: packed element e = bf16 of src[table[e] & 0x3fffffff] (its rounding remainder when bit 30 is set, 0 when
 * table[e] < 0), which also carries folded / concatenated weight layouts (ebfi_amd/weightbank.py). */
size_t ebfi_conv2d_packed_bytes(int Cin, int Cout, int ksize, int transposed);
int ebfi_conv2d_pack_bf16x3(const void *weight, int Cin, int Cout, int ksize, int transposed, void *packed,
                            size_t packed_bytes, void *stream);
int ebfi_pack_table_bf16(const float *src, const int32_t *table, int64_t n, void *out, void *stream);
/* The same [hi | lo] images from one table entry and one gather per (hi, lo) pair.  `table`: per image the source index of every
 * element (negative: structural zero), padded to whole blocks of ebfi_pack_pairs_block() entries; `desc`: four int32 per block --
 * the position in `out` (bf16 elements, low and high half of an int64) of the block's first hi element, the hi -> lo distance in
 * elements, the number of valid entries (even; images start on even positions).  The launch packs the n_active blocks listed
 * in `active`; n_entries (their valid entries) only feeds the profiler's byte count. */
int ebfi_pack_pairs_block(void);
int ebfi_pack_pairs_bf16(const float *src, const int32_t *table, const void *desc, const int32_t *active, int64_t n_active,
                         int64_t n_entries, void *out, void *stream);

/* 3x3, stride 1, padding 1, Cout <= 3, 16 <= Cin <= 64, >= 64 K output pixels (the model's last convolution 64 -> 3 + sigmoid,
 * ExposureDecision's 64 -> 1; reference model_misc/submodules.py:159-200 ConvLayer): Q[(co, tap)][p] = sum_ci w[co][ci][tap] x[ci][p]
 * on the matrix cores (27 of 32 rows used, K = Cin; the input's channel fragments straight from global memory, split into
 * bf16 hi / lo in registers: three products per k-step like every forward convolution here), then out = act(bias + sum_tap
 * Q shifted by the tap) from LDS.  `weight` is the fp32 [Cout, Cin, 3, 3] tensor.  Any other shape: EBFI_ERR_UNSUPPORTED without an
 * error record -- the caller takes ebfi_conv2d_forward_bf16x3 instead. */
int ebfi_conv2d_thin_forward(const void *input, const void *weight, const void *bias, void *output, int B, int Cin, int H, int W,
                             int Cout, int ksize, int stride, int pad, int act, float slope, void *stream);

/* Split-precision convolution on packed weight images with the options hand-scheduled layer chains need
 * (ebfi_amd/rc_fused.py; ResidualControl, reference models/Ours/model_singleframe.py:115-136):
 *   groups      grouped convolution: input [B, groups*Cin_per_group, H, W], output channel co reads the input channels
 *               of group co / (Cout/groups); Cout/groups a multiple of 64 when groups > 1
 *   addend      [B,Cout,Ho,Wo] added before the activation (NULL: none)
 *   mask_y      [B,Cout,Ho,Wo]: the result is multiplied by act'(mask_y) for activation mask_act / mask_slope (NULL: none)
 * out = act(conv(input) + bias + addend) * act'(mask_y); stride 1.  With transposed images it is the data gradient of a
 * layer; addend + mask then turn its output into the PRE-activation gradient of the layer below.
 * Restriction (since ABI 5): with addend or mask_y, `act` and `mask_act` must be none or LeakyReLU -- a sigmoid there returns
 * EBFI_ERR_UNSUPPORTED (the epilogue with extras compiles ONE activation form, LeakyReLU with slope 1 = none; the model never
 * combines a sigmoid layer with them).  Without addend / mask_y every activation is accepted. */
int ebfi_conv2d_packed_x3(const void *input, const void *packed, size_t packed_bytes, const void *bias, void *output,
                          int B, int Cin_per_group, int H, int W, int Cout, int ksize, int pad, int groups, int act,
                          float slope, const void *addend, const void *mask_y, int mask_act, float mask_slope, void *stream);
/* KernelConv -> FAC as ONE kernel (inference).  Replaces, for the pair
 *   filters = LeakyReLU(KernelConv(cat))                 reference models/Ours/model_singleframe.py:161 (ConvLayer 3x3, 2C -> C*K*K)
 *   out     = KernelConv2D(K)(feat, filters)             :162, models/FAC/kernelconv2d/KernelConv2D.py:77-87 (ReplicationPad2d(K//2)
 *                                                        + kernelconv2d_cuda.forward, KernelConv2D_kernel.cu:25-53)
 * the conv launch, the [B, C*K*K, H, W] filter tensor and the FAC launch: the filters exist only in the accumulators of
 * the conv's workgroups, whose epilogue applies them to the replicate-clamped `feat`.
 *   input   [B, Cin, H, W] fp32 (cat([feat, frame_feat]) in the reference model)
 *   packed  split-precision forward images ([hi | lo], bf16 [tap][C*32][Cin16]) of the conv weight re-tiled to 32 rows per
 *           FAC channel: row c*32 + t = weight row c*K*K + t for t < K*K, zero otherwise (ebfi_amd/weightbank.py "facrows")
 *   bias32  [C*32] fp32, same row layout (zeros in the pad rows)
 *   feat    [B, C, H, W] fp32, output [B, C, H, W] fp32; K = 5; W % 4 == 0. */
int ebfi_kernelconv_fac_fused_x3(const void *input, const void *packed, size_t packed_bytes, const void *bias32,
                                 const void *feat, void *output, int B, int Cin, int H, int W, int C, int fac_ksize,
                                 float slope, void *stream);

/* The same fused pair on fp16 operands (round 6; ABI 11): one matrix-core product per tap.  `input` fp32 NCHW, multiplied by
 * in_slot[0] (a power of two the caller sets from the tensor right before the launch) while it is staged, |max| recorded in
 * in_slot -- or, input_is_c16 = 1, the c16 image of that tensor written by ebfi_to_c16 with in_slot's scale (Cin % 16 == 0: half
 * the bytes per staged chunk; every one of the C / 2 output-channel blocks stages the whole input); `packed16`: the "facrows" fp16 image [tap][C*32][K16] scaled by w_slot[0] (ebfi_pack_table_f16).  Replaces the same
 * reference lines as ebfi_kernelconv_fac_fused_x3 (model_singleframe.py:161-162, KernelConv2D.py:82-87,
 * KernelConv2D_kernel.cu:25-53) for inference. */
int ebfi_kernelconv_fac_fused_f16(const void *input, int input_is_c16, const void *packed16, size_t packed_bytes,
                                  const void *bias32, const void *feat, void *output, int B, int Cin, int H, int W, int C,
                                  int fac_ksize, float slope, void *in_slot, const void *w_slot, void *stream);
/* ------------------------------------------------------------------ fp16 single-product backward (training step)
 * The data gradient and the weight gradient of the 3x3 layers with ONE fp16 MFMA per product (the forward keeps the
 * split-precision kernels: DESIGN.md section 4).  Every operand is scaled by a power of two kept in a device SLOT of
 * 64 floats (256 bytes): slot[0] = scale, slot[32] = running |max| of the values staged through it (separate cache lines);
 * kernels apply slot[0] and atomically raise slot[32]; slot i of a book starts at slots + 64 i;
 * ebfi_f16_scales_finish (once per step, after the backward pass) turns the maxima of all `n` slots into the next step's
 * scales (|max| * scale in [2, 4)), clears them, and sets flag[0] when a value was not finite or |max| * scale could
 * have left the fp16 range.  A new slot is initialised by the caller (ebfi_amd/f16scale.py calibrates it just in time).
 *   ebfi_pack_table_f16      fp16 weight images from the index table of ebfi_pack_table_bf16 (hi entries); images start on
 *                            256-element boundaries, elements [256 k, 256 k + 256) are scaled by slot block_slot[k]
 *   ebfi_conv2d_packed_f16   ebfi_conv2d_packed_x3 on an fp16 image (3x3, pad 1, W % 4 == 0): out = act(conv / (in_scale *
 *                            w_scale) + bias + addend) * act'(mask_y); with transposed images: the data gradient
 *   ebfi_conv2d_backward_weight_f16g   ebfi_conv2d_backward_weight_x3g / _ex (act'(saved_output) folded, optional
 *                            grad_preact_out) with fp16 operands; Cin_per_group a multiple of 64 */
int ebfi_f16_scales_finish(void *slots, int n, void *flag, void *stream);
int ebfi_pack_table_f16(const float *src, const int32_t *table, int64_t n, void *out, const int32_t *block_slot,
                        void *slots, void *stream);
int ebfi_conv2d_packed_f16(const void *input, const void *packed16, size_t packed_bytes, const void *bias, void *output,
                           int B, int Cin_per_group, int H, int W, int Cout, int ksize, int pad, int groups, int act,
                           float slope, const void *addend, const void *mask_y, int mask_act, float mask_slope,
                           void *in_slot, const void *w_slot, void *stream);
int ebfi_conv2d_backward_weight_f16g(const void *input, const void *grad_output, const void *saved_output,
                                     void *grad_weight, void *grad_bias, void *grad_preact_out, int B,
                                     int Cin_per_group, int H, int W, int Cout, int ksize, int pad, int groups, int act,
                                     float slope, void *x_slot, void *g_slot, void *workspace,
                                     size_t workspace_bytes, void *stream);
/* _ex: grad_preact_is_c16 != 0 writes grad_preact_out (grad_output * act'(saved_output)) as a c16 image scaled by g_slot's scale
 * (see "fp16 operand STORAGE" below) for ebfi_conv2d_packed_f16_c16 to stage; needs an activation, Cout % 16 == 0, 3x3 / pad 1,
 * W % 4 == 0 and 16-byte aligned tensors (EBFI_ERR_UNSUPPORTED otherwise) */
int ebfi_conv2d_backward_weight_f16g_ex(const void *input, const void *grad_output, const void *saved_output,
                                        void *grad_weight, void *grad_bias, void *grad_preact_out, int grad_preact_is_c16, int B,
                                        int Cin_per_group, int H, int W, int Cout, int ksize, int pad, int groups, int act,
                                        float slope, void *x_slot, void *g_slot, void *workspace,
                                        size_t workspace_bytes, void *stream);
/* ------------------------------------------------------------------ fp16 operand STORAGE of the backward pass (round 4)
 * Layout "c16": a tensor [B, C, H, W] (C % 16 == 0, W % 4 == 0) as fp16 [B][C/16][H][2][W][8] -- 16-channel blocks; an image
 * row holds the channels 0..7 of its W pixels, then the channels 8..15 -- multiplied by the power-of-two scale in slot[0] of
 * its scale slot (ebfi_f16_scales_finish).  It is the staging
 * layout of both fp16 backward kernels: their producers copy 16-byte pieces instead of converting fp32 NCHW planes, half
 * the bytes.  The WRITER of an image applies the scale and records |max| into the slot; readers only read the scale.
 * Replaces, inside ResidualControl's backward chain (models/Ours/model_singleframe.py:115-136), the fp32 tensors autograd
 * would hand from layer to layer.
 *   ebfi_to_c16                        fp32 [B,C,HW] -> image (optionally times LeakyReLU'(mask_y): a pre-activation gradient)
 *   ebfi_conv2d_packed_x3_c16          ebfi_conv2d_packed_x3 writing its output also as an image (out16, slot16)
 *   ebfi_conv2d_packed_f16_c16         ebfi_conv2d_packed_f16 reading an image (input_is_c16 = 1; 2 = planar fp16; scale in in_slot) and / or
 *                                      writing its output as one (out16 / slot16; `output` may then be NULL); mask_is_c16: mask_y is
 *                                      the c16 image of the mask tensor (its signs are read) instead of the fp32 tensor
 *   ebfi_conv2d_backward_weight_f16c   weight / bias gradient from the images of the input and of the pre-activation gradient
 *   ebfi_scale_residual_cat_forward_c16 / _backward_c16   the fused ResidualControl stages writing images: forward out + out16;
 *                                      backward [grad_a0 | grad_a1] * LeakyReLU'(a) as ONE image of 2C channels, grad_x fp32,
 *                                      scale gradients as per-slice partial sums [slices][B][C] (summed in order by the caller) */
int ebfi_to_c16(const float *src, const float *mask_y, float mask_slope, void *dst16, void *slot, int B, int C, int H, int W,
                void *stream);
/* Round 6 (ABI 14): the image of cat([src0, src1], 1) -- [B, C0 + C1, H, W] -- written from its two parts: the concatenated fp32 tensor
 * of Modification (`torch.cat([ev, FrameTensor], 1)`, model_singleframe.py:159-160) is never materialised when its only consumer, the
 * 128 -> 1600 KernelConv of the training step, reads the image.  C0, C1 multiples of 8, C0 + C1 a multiple of 16; same bits as
 * ebfi_to_c16 of the concatenation. */
int ebfi_to_c16_cat2(const float *src0, int C0, const float *src1, int C1, void *dst16, void *slot, int B, int H, int W, void *stream);
int ebfi_conv2d_packed_x3_c16(const void *input, const void *packed, size_t packed_bytes, const void *bias, void *output,
                              int B, int Cin_per_group, int H, int W, int Cout, int ksize, int pad, int groups, int act,
                              float slope, const void *addend, const void *mask_y, int mask_act, float mask_slope,
                              void *out16, void *slot16, int out16_planar, void *stream);
int ebfi_conv2d_packed_f16_c16(const void *input, int input_is_c16, const void *packed16, size_t packed_bytes,
                               const void *bias, void *output, int B, int Cin_per_group, int H, int W, int Cout, int ksize,
                               int pad, int groups, int act, float slope, const void *addend, const void *mask_y,
                               int mask_act, float mask_slope, void *in_slot, const void *w_slot, void *out16,
                               void *slot16, int out16_planar, int mask_is_c16, void *stream);
/* Round 6 (ABI 13): the two packed convolutions with the fp32 output stored THROUGH PixelShuffle(2) (out_layout 1: `output` is
 * [B, Cout/4, 2H, 2W], channel 4c + 2py + px of pixel (y, x) at (c, 2y + py, 2x + px); Cout % 4 == 0) or through its inverse
 * (out_layout 2: [B, 4*Cout, H/2, W/2]; H, W even); 0 = the plain layout.  3x3 same-padded layers on the wave-specialised kernels
 * (W % 4 == 0, Cout > 32, 16-byte aligned input), no groups, no addend, no fp16 side output.  Replaces the PixelShuffle copy of the
 * reconstruction head (models/Ours/model_singleframe.py:257-260: conv 64 -> 256, nn.PixelShuffle(2), LeakyReLU) and its backward:
 *   forward   ebfi_conv2d_packed_x3_shuffled(.., act = LeakyReLU, out_layout 1) writes what the next layer reads;
 *   backward  ebfi_conv2d_packed_f16_shuffled on that next layer's TRANSPOSED fp16 image with mask_y = that layer's own input (the
 *             shuffled activation, natural layout of this launch), out_layout 2: the pre-activation gradient of the 64 -> 256
 *             convolution in ITS layout.  mask_y / mask_act / mask_slope as in ebfi_conv2d_packed_f16_c16 (fp32 mask tensor). */
int ebfi_conv2d_packed_x3_shuffled(const void *input, const void *packed, size_t packed_bytes, const void *bias, void *output,
                                   int B, int Cin, int H, int W, int Cout, int act, float slope, int out_layout, void *stream);
int ebfi_conv2d_packed_f16_shuffled(const void *input, int input_is_c16, const void *packed16, size_t packed_bytes,
                                    const void *bias, void *output, int B, int Cin, int H, int W, int Cout, int act, float slope,
                                    const void *mask_y, int mask_act, float mask_slope, void *in_slot, const void *w_slot,
                                    int out_layout, void *stream);
int ebfi_conv2d_backward_weight_f16c(const void *input16, const void *grad16, int grad_is_planar, void *grad_weight,
                                     void *grad_bias, int B, int Cin_per_group, int H, int W, int Cout, int groups,
                                     const void *x_slot, const void *g_slot, void *workspace, size_t workspace_bytes,
                                     void *stream);
/* n (1..4) weight gradients over the SAME [B, H, W] pixels as ONE launch + one reduction (the three layers of a ResidualControl
 * round, models/Ours/model_singleframe.py:127-133): arguments are arrays of n entries; every layer must be exactly two 64 x 64
 * blocks (128 x 64, 64 x 128, or 2 groups of 64 x 64) -- otherwise EBFI_ERR_UNSUPPORTED and the caller uses the per-layer entry.
 * A third of the partial-sum slab traffic and of the start-up per layer. */
size_t ebfi_conv2d_backward_weight_f16c_batch_workspace(int n, const int *Cin_per_group, const int *Cout);
int ebfi_conv2d_backward_weight_f16c_batch(int n, const void *const *input16, const void *const *grad16, void *const *grad_weight,
                                           void *const *grad_bias, const int *Cin_per_group, const int *Cout, const int *groups,
                                           void *const *x_slot, void *const *g_slot, int B, int H, int W, void *workspace,
                                           size_t workspace_bytes, void *stream);
/* n weight / bias gradients with a geometry of their own each, in ceil(n / 16) launches (+ as many reduction launches):
 * the PURE weight gradients of a training step -- fp32 `input` / `grad_output`, the incoming gradient already that of the
 * pre-activation -- which nothing in the backward pass waits for, deferred to its end (ebfi_amd/wgradqueue.py).  Arguments are
 * arrays of n entries.  Every item must be what ebfi_conv2d_backward_weight_f16g_ex runs on its pixel-major kernel with act = 0:
 * ksize 3, stride 1, pad 1, groups 1, W % 4 == 0, Cin >= 16, 16-byte aligned input and grad_output, Cout > 4 on large maps (the
 * thin layers have kernels of their own); one item outside that returns EBFI_ERR_UNSUPPORTED for the whole call and launches
 * nothing.  x_slot / g_slot as there (scale applied and |max| recorded while staging; NULL = unscaled); grad_bias entries may be
 * NULL.  Every item keeps the split count of ebfi_conv2d_backward_weight_f16g_ex, whatever shares the launch with it: each
 * result is bit-identical to that entry point's.  Deterministic. */
size_t ebfi_conv2d_backward_weight_f16g_multi_workspace(int n, const int *B, const int *Cin, const int *H, const int *W, const int *Cout);
int ebfi_conv2d_backward_weight_f16g_multi(int n, const void *const *input, const void *const *grad_output, void *const *grad_weight,
                                           void *const *grad_bias, const int *B, const int *Cin, const int *H, const int *W,
                                           const int *Cout, const int *ksize, const int *stride, const int *pad, const int *groups,
                                           void *const *x_slot, void *const *g_slot, void *workspace, size_t workspace_bytes,
                                           void *stream);
/* The 1600-channel tensors of the KernelConv -> FAC pair in the TRAINING step (reference
 * models/Ours/model_singleframe.py:161-162, KernelConv2D_kernel.cu:25-150): the filters and grad_kernel as PLANAR fp16
 * [B, C*K*K, Ho, Wo] scaled by a slot's power of two -- the layout the FAC kernels stream plane by plane.  The 128 -> 1600
 * convolution writes the filters in that form (ebfi_conv2d_packed_x3_c16 with out16_planar, output NULL), the FAC forward /
 * backward read them and the backward writes grad_kernel (times the LeakyReLU derivative) likewise; the weight / data
 * gradient of the convolution stage the planes (ebfi_conv2d_backward_weight_f16c grad_is_planar, ebfi_conv2d_packed_f16_c16
 * input_is_c16 = 2).  No fp32 [B, 1600, h, w] tensor is written or read. */
/* input_is_unpadded (round 5): `input` (and grad_input) are the UNPADDED [B, C, Ho, Wo] tensors and the replicate padding of
 * KernelConv2D.py:82-86 (nn.ReplicationPad2d(K / 2)) is applied inside the kernels -- clamped reads in the forward; in the
 * backward clamped reads plus the padding's ADJOINT folded into grad_input with a fixed summation order (no atomics: torch's
 * replication_pad2d_backward adds atomically).  0: `input` is the padded [B, C, Ho+K-1, Wo+K-1] tensor as before. */
int ebfi_fac_forward_p16(const float *input, int input_is_unpadded, const void *filters16, const void *f_slot, float *output, int B,
                         int C, int Ho, int Wo, int K, void *stream);
int ebfi_fac_backward_p16(const float *input, int input_is_unpadded, const void *filters16, const void *f_slot,
                          const float *grad_output, float *grad_input, void *grad_kernel16, void *g_slot, float kernel_leaky_slope,
                          int B, int C, int Ho, int Wo, int K, void *stream);
int ebfi_scale_residual_cat_forward_c16(const float *a0, const float *s0, const float *a1, const float *s1, const float *x,
                                        float *out, void *out16, void *slot, int B, int C, int H, int W,
                                        int64_t a_batch_stride, void *stream);
int ebfi_scale_residual_cat_backward_slices(void);
int ebfi_scale_residual_cat_backward_c16(const float *grad_out, const float *a0, const float *s0, const float *a1,
                                         const float *s1, void *grad_a16, void *slot, float *grad_x, float *grad_s0_part,
                                         float *grad_s1_part, int B, int C, int H, int W, int64_t a_batch_stride,
                                         float mask_slope, void *stream);
/* ... with `a` as the c16 image of [a0 | a1] (2C channels, scale in a_slot) written by ebfi_conv2d_packed_x3_rc (round 5). */
int ebfi_scale_residual_cat_backward_c16a(const float *grad_out, const void *a16, const void *a_slot, const float *s0, const float *s1,
                                          void *grad_a16, void *slot, float *grad_x, float *grad_s0_part, float *grad_s1_part, int B,
                                          int C, int H, int W, float mask_slope, void *stream);
/* The grouped second-layer convolution of a ResidualControl round with the round's tail in its epilogue
 * (models/Ours/model_singleframe.py:127-133): a = LeakyReLU(conv3x3(input) + bias); pre16 = c16 image of a (scale / |max| in
 * pre_slot); output[b, co] = a * post_scale[b, co] + post_res[b, co % res_channels] -- the exposure- / time-scaled residual and
 * concatenation `cat(s_ex * a0 + x, s_t * a1 + x)` -- and out16 = c16 image of output.  Replaces the separate
 * ebfi_scale_residual_cat_forward_c16 launch; no fp32 `a` is written.  3x3, same padding, 64-channel blocks, W % 4 == 0.
 * Inference form: pre16, pre_slot, out16 and slot16 all NULL -- only `output` is written (replaces the launch of
 * ebfi_scale_residual_cat_forward_ex after the convolution, and the fp32 `a` between them). */
int ebfi_conv2d_packed_x3_rc(const void *input, const void *packed, size_t packed_bytes, const void *bias, void *output, int B,
                             int Cin_per_group, int H, int W, int Cout, int groups, float slope, const void *post_scale,
                             const void *post_res, int res_channels, void *pre16, void *pre_slot, void *out16, void *slot16,
                             void *stream);
/* weight / bias gradient of such a (grouped) convolution from a pre-activation gradient: grad_weight
 * [Cout, Cin_per_group, k, k]; workspace as ebfi_conv2d_backward_weight_workspace(B, Cin_per_group, H, W, Cout, k, 1, pad) */
int ebfi_conv2d_backward_weight_x3g(const void *input, const void *grad_output, void *grad_weight, void *grad_bias,
                                    int B, int Cin_per_group, int H, int W, int Cout, int ksize, int pad, int groups,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ event voxel binning
 * xs, ys, ts: float64[n] device (ts sorted, normalised as h5dataset.py:334), ps: float32[n].
 * out: float32 [2, bins, H, W], fully overwritten (index 0 = positive, 1 = negative counts).
 * Bit-exact with events_to_stack incl. its shared-edge and out-of-range behaviour.
 * workspace: ebfi_events_workspace(bins) bytes. */
size_t ebfi_events_workspace(int bins);
int ebfi_events_to_stack(const double *xs, const double *ys, const double *ts, const float *ps,
                         int64_t n, int bins, int H, int W, float *out,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ blur-level maps
 * frame: float32 [B,3,H,W] contiguous in [0,1]; out: float32 [B,1,H,W]. */
int ebfi_frame2lap(const float *frame, float *out, int B, int H, int W, void *stream);
int ebfi_frame2dcp(const float *frame, float *out, float *scratch /* [B,H,W] */, int B, int H, int W,
                   int window, void *stream);

/* ------------------------------------------------------------------ scalar-conditioned channel scales
 * ResidualControl's Conv1[i](Ex) / Conv2[i](T) (models/Ours/model_singleframe.py:85-94, :127-129: ConvLayer(k=1) + LeakyReLU on a
 * [B,K,1,1] input, reference submodules.py:159-200) for a BANK of S such layers in one launch:
 *   out[s][b][c] = leaky_relu(bias_s[c] + sum_k v[b][k] * weight_s[c][k], slope)        v [B,K], weight_s [C,K], out [S,B,C]
 * weights / biases: host arrays of S device pointers (the layers' own parameter tensors; bias entries may be NULL); they are
 * copied into the kernel arguments, so a captured launch keeps them.  S <= 32, K <= 8, S*B*C <= 2^20.
 * backward: grad_weight [S,C,K], grad_bias [S,C], grad_v [B,K] (each may be NULL), all fully overwritten, fixed summation
 * order (bit-reproducible); `out` is the forward's output (its sign selects the LeakyReLU derivative). */
int ebfi_scalar_conv_forward(const float *v, const void *const *weights, const void *const *biases, float *out, int S, int B,
                             int K, int C, float slope, void *stream);
int ebfi_scalar_conv_backward(const float *v, const void *const *weights, const float *out, const float *grad_out,
                              float *grad_weight, float *grad_bias, float *grad_v, int S, int B, int K, int C, float slope,
                              void *stream);

/* ------------------------------------------------------------------ fused stages between the convolutions
 * One round of ResidualControl (models/Ours/model_singleframe.py:124-134):
 *   out[:, :C] = s0[b,c] * a0 + x,  out[:, C:] = s1[b,c] * a1 + x      (a0/a1/x [B,C,H,W], s0/s1 [B,C], out [B,2C,H,W])
 * backward is its adjoint (grad_s* reduced per plane in fixed order).  HW = H*W, a multiple of 4.
 * x == NULL drops the residual (then grad_x == NULL), s1 == NULL means s1 = 1 (then a1 / grad_s1 are not read / written
 * by the backward): cat([atten * ev, bl]) of ExposureDecision (model_singleframe.py:68-72) is the same stage. */
int ebfi_scale_residual_cat_forward(const float *a0, const float *s0, const float *a1, const float *s1, const float *x,
                                    float *out, int B, int C, int64_t HW, void *stream);
int ebfi_scale_residual_cat_backward(const float *grad_out, const float *a0, const float *s0, const float *a1,
                                     const float *s1, float *grad_a0, float *grad_a1, float *grad_x,
                                     float *grad_s0, float *grad_s1, int B, int C, int64_t HW, void *stream);

/* The same stage with a0 / a1 (and grad_a0 / grad_a1) given as channel slices of wider [B, *, H, W] tensors (batch strides
 * in elements, multiples of 4).  mask_leaky != 0: a0 / a1 are LeakyReLU(mask_slope) outputs and grad_a0 / grad_a1 leave
 * multiplied by that activation's derivative, i.e. as gradients of the PRE-activations. */
int ebfi_scale_residual_cat_forward_ex(const float *a0, const float *s0, const float *a1, const float *s1, const float *x,
                                       float *out, int B, int C, int64_t HW, int64_t a_batch_stride, void *stream);
int ebfi_scale_residual_cat_backward_ex(const float *grad_out, const float *a0, const float *s0, const float *a1,
                                        const float *s1, float *grad_a0, float *grad_a1, float *grad_x, float *grad_s0,
                                        float *grad_s1, int B, int C, int64_t HW, int64_t a_batch_stride,
                                        int64_t grad_a_batch_stride, int mask_leaky, float mask_slope, void *stream);

/* out[plane] = mean over HW of a*b for contiguous [planes, HW] maps (AdaptiveAvgPool2d(1) of a product: the event / blur
 * correlation of ExposureDecision, model_singleframe.py:66-68) and its adjoint.  HW a multiple of 4. */
int ebfi_prodmean_forward(const float *a, const float *b, float *out, int64_t planes, int64_t HW, void *stream);
int ebfi_prodmean_backward(const float *a, const float *b, const float *grad_out, float *grad_a, float *grad_b,
                           int64_t planes, int64_t HW, void *stream);

/* Sparse 0/1 linear map: out[i] = sum_{r<R} src[idx[i*R+r]], negative indices skipped.  Carries the weight
 * re-layouts that turn the depth-2 Conv3d / ConvTranspose3d of the detail branch (models/model_misc/resnet_3D.py,
 * model_singleframe.py:170-223) into 2-D convolutions, and their adjoints. */
int ebfi_gather_sum(const float *src, const int32_t *idx, float *out, int64_t n_out, int R, void *stream);
/* n of them (arrays of n entries) in ceil(n / 48) launches; bit-identical to n calls of ebfi_gather_sum. */
int ebfi_gather_sum_multi(int n, const float *const *src, const int32_t *const *idx, float *const *out, const int64_t *n_out,
                          const int *R, void *stream);

/* ------------------------------------------------------------------ squeeze-excite gate of the detail branch
 * SEGating (models/model_misc/resnet_3D.py:89-105) fused with what follows it: out = act(x * sigmoid(W mean(x) + b) (+ res)).
 * x, res, out: [B*C planes][N] contiguous fp32 (a [B,C,D,H,W] tensor as it stands), N % 4 == 0, B*C <= 4096;
 * weight [C,C] (the 1x1x1 conv), bias [C] or NULL; act: 0 none, 1 LeakyReLU(slope) (slope 0 = ReLU).
 * forward writes mean [B*C] and gate [B*C] for the backward; both directions take a workspace of
 * ebfi_se_gate_workspace(B, C, N) floats (slice sums of the plane reductions); grad_res / grad_bias may be NULL; `out` may be
 * NULL when act == 0 (backward).  Two launches each way, deterministic (fixed-order reductions). */
size_t ebfi_se_gate_workspace(int B, int C, int64_t N);
int ebfi_se_gate_forward(const float *x, const float *weight, const float *bias, const float *res, float *out, float *mean,
                         float *gate, float *workspace, int B, int C, int64_t N, int act, float slope, void *stream);
int ebfi_se_gate_backward(const float *grad_out, const float *out, const float *x, const float *weight, const float *gate,
                          const float *mean, float *grad_x, float *grad_res, float *grad_weight, float *grad_bias,
                          float *workspace, int B, int C, int64_t N, int act, float slope, void *stream);

/* Round 6 (ABI 12): the same gate behind a transposed convolution whose output has NOT been pixel-shuffled yet -- upConv3D of the
 * detail branch (model_singleframe.py:200-223, resnet_3D / model_3DUnet upConv3D: ConvTranspose3d (3,4,4)/(1,2,2) -> SEGating ->
 * LeakyReLU), run here as a 3x3 convolution to 8*C channels.  x: that convolution's output [B, 8*C, h, w] (channel = (c, d, py, px));
 * out / grad_out: [B, C, 2, 2h, 2w]; grad_x in x's layout.  The gate kernels address x through the shuffle: the PixelShuffle copy
 * of the stage's largest tensor (forward and backward) never runs.  w even; no residual input. */
int ebfi_se_gate_forward_ps(const float *x, const float *weight, const float *bias, float *out, float *mean, float *gate,
                            float *workspace, int B, int C, int h, int w, int act, float slope, void *stream);
int ebfi_se_gate_backward_ps(const float *grad_out, const float *out, const float *x, const float *weight, const float *gate,
                             const float *mean, float *grad_x, float *grad_weight, float *grad_bias, float *workspace, int B, int C,
                             int h, int w, int act, float slope, void *stream);

/* ------------------------------------------------------------------ GroupNorm (exposure-decision head)
 * nn.GroupNorm(groups, C) on contiguous NCHW fp32 (reference models/Ours/model_singleframe.py:36,66-67).
 * HW = H*W must be a multiple of 4.  mean / rstd [B*groups] are written by forward and read by backward.
 * workspace: ebfi_groupnorm_workspace(B, C) bytes for forward, that + 2*B*groups*4 for backward.
 * gamma / beta / grad_gamma / grad_beta may be NULL.  Deterministic (fixed-order double-precision sums). */
size_t ebfi_groupnorm_workspace(int B, int C);
int ebfi_groupnorm_forward(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *rstd,
                           int B, int C, int64_t HW, int groups, float eps,
                           void *workspace, size_t workspace_bytes, void *stream);
int ebfi_groupnorm_backward(const float *grad_y, const float *x, const float *gamma, const float *mean,
                            const float *rstd, float *grad_x, float *grad_gamma, float *grad_beta,
                            int B, int C, int64_t HW, int groups,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ExposureDecision head (models/Ours/model_singleframe.py:66-72) for contiguous [B,C,H,W] maps ev, bl and ONE GroupNorm
 * (gamma, beta [C], `groups`, eps) applied to both:
 *   atten[B*C] = sigmoid(mean_HW(GN(ev) * GN(bl)));   out[B,2C,H,W] = cat([ev * atten, bl], 1).
 * GN is affine per plane, so the pooled product follows from five plane moments: one pass over the maps, no normalised
 * map is written.  forward also writes `stats` (B*C*5 + B*groups*4 doubles: plane means of ev, ev^2, bl, bl^2, ev*bl,
 * then (mean, rstd) of both maps per group) for backward, which returns the gradients of the whole head
 *   grad_ev, grad_bl [B,C,H,W], grad_gamma, grad_beta [C] (may be NULL)
 * from grad_out [B,2C,H,W] in one reduction + one elementwise pass (closed form in the moments).
 * HW % 4 == 0, C % groups == 0, C <= 1024; workspace: ebfi_ed_head_workspace(B, C, HW) bytes, 16-byte aligned (it holds
 * double partial sums).  Deterministic. */
size_t ebfi_ed_head_workspace(int B, int C, int64_t HW);
int ebfi_ed_head_forward(const float *ev, const float *bl, const float *gamma, const float *beta, float *out, float *atten,
                         double *stats, int B, int C, int64_t HW, int groups, float eps,
                         void *workspace, size_t workspace_bytes, void *stream);
int ebfi_ed_head_backward(const float *grad_out, const float *ev, const float *bl, const float *gamma, const float *beta,
                          const float *atten, const double *stats, float *grad_ev, float *grad_bl, float *grad_gamma,
                          float *grad_beta, int B, int C, int64_t HW, int groups,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ loss image operators
 * 5x5 binomial blur ([1,4,6,4,1]/16 twice, times `factor`) with reflect padding over `planes` contiguous
 * H x W planes: the GaussianConv of the reference's Laplacian-pyramid loss (loss/restore.py:149-163).
 * backward is its exact adjoint.  H, W >= 3. */
int ebfi_gauss5_forward(const float *input, float *output, int64_t planes, int H, int W, float factor, void *stream);
int ebfi_gauss5_backward(const float *grad_output, float *grad_input, int64_t planes, int H, int W, float factor,
                         void *stream);

/* Census (Ternary, 7x7) loss of loss/restore.py:108-145 on [B,C,H,W] fp32 images, gray = channel mean.
 * forward writes ebfi_census_partials(B,H,W) per-tile sums; loss = sum(partial) / (B*H*W) (summed by the caller
 * in fixed order -> deterministic).  backward: grad_x = grad_loss[0] * d loss / d x; y is a constant (the
 * reference detaches the target transform, restore.py:138). */
int64_t ebfi_census_partials(int B, int H, int W);
int ebfi_census_forward(const float *x, const float *y, float *partial, int B, int C, int H, int W, void *stream);
int ebfi_census_backward(const float *x, const float *y, const float *grad_loss, float *grad_x,
                         int B, int C, int H, int W, void *stream);

/* The two census terms of a training step (two predictions, one target) in one launch each way.  forward: partial holds
 * 2 * ebfi_census_partials(B,H,W) floats, the per-tile sums of (xa, y) then of (xb, y), each exactly what ebfi_census_forward
 * writes; a one-workgroup launch then adds them in a fixed order: loss[0] = wa * sum_a / (B*H*W) + wb * sum_b / (B*H*W).
 * backward: grad_xa / grad_xb = what ebfi_census_backward gives for the 1-element gradient grad_loss[0] * wa / * wb, bit for
 * bit.  xb == NULL: one prediction (loss[0] = wa * sum_a / (B*H*W); grad_xb is not touched). */
int ebfi_census_pair_forward(const float *xa, const float *xb, const float *y, float wa, float wb, float *partial, float *loss,
                             int B, int C, int H, int W, void *stream);
int ebfi_census_pair_backward(const float *xa, const float *xb, const float *y, float wa, float wb, const float *grad_loss,
                              float *grad_xa, float *grad_xb, int B, int C, int H, int W, void *stream);

/* Laplacian-pyramid L1 term of the training loss for up to two predictions against one target
 * (loss/restore.py:166-213 LaplacianPyramid + LaplacianLoss: sum_i 2^i * L1sum(lap_i(pred), lap_i(target)), `levels` = 5;
 * combined for (Sharp, SharpPre) with the coefficients of train_ours.py:258-268).  The pyramid operators are linear,
 * so the library builds ONE pyramid of [pred_a - target ; pred_b - target] (planes_per_term = B*C planes of H x W each;
 * pred_b may be NULL).  forward fills `workspace` (ebfi_laploss_workspace_floats(planes, ...) floats, planes = 1 or 2
 * x planes_per_term) and writes ebfi_laploss_partials(planes, ...) block sums:
 *   loss = coef_a * Lap(pred_a, target) + coef_b * Lap(pred_b, target) = sum(partial)   (summed by the caller, fixed order).
 * backward turns the workspace left by forward (consumed in place: once per forward) into
 *   grad_pred[planes, H, W] = grad_loss[0] * d loss / d [pred_a ; pred_b].
 * H, W multiples of 2^(levels-1), >= 3 pixels on the coarsest blurred level, 2 <= levels <= 8. */
int64_t ebfi_laploss_workspace_floats(int64_t planes, int H, int W, int levels);
int64_t ebfi_laploss_partials(int64_t planes, int H, int W, int levels);
int ebfi_laploss_forward(const float *pred_a, const float *pred_b, const float *target, float coef_a, float coef_b,
                         float *workspace, float *partial, int64_t planes_per_term, int H, int W, int levels, void *stream);
int ebfi_laploss_backward(const float *grad_loss, float *workspace, float *grad_pred, int64_t planes, int H, int W,
                          int levels, void *stream);

/* Adjoints of nn.ReflectionPad2d(pad) (the detail branch's output conv: ReflectionPad2d(3) + 7x7 convolution,
 * models/Ours/model_singleframe.py:207; replicate = 0) and nn.ReplicationPad2d(pad) (the FAC module,
 * models/FAC/kernelconv2d/KernelConv2D.py:82-86; replicate = 1): grad_padded [planes, H+2*pad, W+2*pad] -> grad_input
 * [planes, H, W] as a gather in a fixed order (bit-reproducible; torch's backward of either pad accumulates with atomics).
 * Reflection needs pad < H, W. */
int ebfi_pad2d_backward(const float *grad_padded, float *grad_input, int64_t planes, int H, int W, int pad, int replicate, void *stream);

/* Adam update (torch.optim.Adam of train_ours.py:276-277, amsgrad / weight decay off as in config/train_ours.yml:59-65)
 * over one flat fp32 buffer of n elements, in place: exp_avg <- exp_avg + (1-beta1)(grad - exp_avg);
 * exp_avg_sq <- beta2 exp_avg_sq + (1-beta2) grad^2; param <- param - lr/(1-beta1^t) * exp_avg / (sqrt(exp_avg_sq)/sqrt(1-beta2^t) + eps)
 * with t = step[0] (a device scalar holding the ALREADY incremented step count: no host synchronisation).
 * All buffers 16-byte aligned. */
int ebfi_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, const float *step, int64_t n,
                   double lr, double beta1, double beta2, double eps, void *stream);
/* Same update, guarded: when guard[0] != 0 (set by ebfi_f16_scales_finish: an fp16 operand of this step's backward pass
 * left its range) nothing is updated, step[0] is decremented again and guard[1] counts the skipped step.  guard may be NULL.
 * flag (optional, needs guard): one device float, the ranks' guard flags summed by the gradient all-reduce (ebfi_grad_gather
 * wrote this rank's into the wire buffer): anything but an exact 0 skips the step too and sets guard[0] = 1, so every rank
 * of a data-parallel job takes the same branch without a collective of its own for the flag. */
int ebfi_adam_step_guarded(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, int64_t n,
                           double lr, double beta1, double beta2, double eps, int *guard, const float *flag, void *stream);

/* The optimiser section of the training config (the reference: eval(config['optimizer']['name'])(params,
 * **config['optimizer']['args']), train_ours.py:770-771) as ONE launch over the flat fp32 buffer of n elements, in place.
 * Hyper-parameters travel by value, so a scheduler's new lr needs no recapture of a graph.  grad is only read.
 *   kind EBFI_OPTIM_ADAM  torch.optim.Adam / AdamW.  state0 = exp_avg, state1 = exp_avg_sq, state2 = max_exp_avg_sq (read and
 *        written only with EBFI_OPTIM_AMSGRAD, NULL otherwise), step = device scalar holding the ALREADY incremented count.
 *        weight_decay != 0: grad' = grad + weight_decay param before the moments (L2, torch.optim.Adam), or with
 *        EBFI_OPTIM_DECOUPLED_DECAY param <- param (1 - lr weight_decay) before the update (torch.optim.AdamW).
 *        EBFI_OPTIM_AMSGRAD: max_exp_avg_sq <- max(max_exp_avg_sq, exp_avg_sq), and the denominator is built from it.
 *        Bias corrections in double precision as in ebfi_adam_step.  momentum / dampening are ignored.  Without weight decay
 *        and AMSGrad this IS ebfi_adam_step_guarded: the same kernel, the same bits.
 *   kind EBFI_OPTIM_SGD   torch.optim.SGD.  d = grad + weight_decay param; with momentum != 0 (state0 = momentum_buffer,
 *        step as above): buf <- d when step[0] == 1 (the first APPLIED step: a skipped step takes the count back),
 *        buf <- momentum buf + (1 - dampening) d afterwards; d <- d + momentum buf with EBFI_OPTIM_NESTEROV (needs
 *        momentum > 0 and dampening == 0, as torch does), d <- buf otherwise; param <- param - lr d.  With momentum == 0
 *        neither state0 nor step is touched (both may be NULL).  beta1 / beta2 / eps, state1 and state2 are ignored.
 * guard / flag: exactly as in ebfi_adam_step_guarded -- a skipped step writes no parameter and no state element, takes the
 * step word back, counts in guard[1], and guard[0] becomes 1 when the flag said skip.
 * A flag of the other kind, or an unknown one, is EBFI_ERR_ARG; an unknown kind EBFI_ERR_UNSUPPORTED.  Every buffer that is
 * used must be 16-byte aligned.  Bytes moved per launch: 4 n x (3 plain SGD, 5 SGD with momentum, 7 Adam, 9 AMSGrad). */
#define EBFI_OPTIM_ADAM 0
#define EBFI_OPTIM_SGD 1
#define EBFI_OPTIM_DECOUPLED_DECAY 1
#define EBFI_OPTIM_AMSGRAD 2
#define EBFI_OPTIM_NESTEROV 4
int ebfi_optim_step(int kind, int flags, float *param, const float *grad, float *state0, float *state1, float *state2,
                    float *step, int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                    double momentum, double dampening, int *guard, const float *flag, void *stream);

/* Total norm of the flat gradient and the clipping coefficient of torch.nn.utils.clip_grad_norm_, both left ON THE DEVICE
 * (no host synchronisation): grad float32 [n], 16-byte aligned, only read; out float32 [2].
 *   out[0] = (float)sqrt(sum g^2) (EBFI_NORM_L2) or max |g| (EBFI_NORM_INF)
 *   out[1] = c = (float)max_norm / (out[0] + 1e-6f), then c > 1 ? 1 : c -- float32, nothing contracted: torch's arithmetic,
 *            also for a non-finite norm (NaN norm -> NaN coefficient, infinite norm -> 0)
 * Two launches.  The first gives every workgroup one chunk of EBFI_GRAD_NORM_CHUNK elements (16-byte loads; the n % 4 last
 * elements by scalar loads in the workgroup that owns them): every value is widened to float64, squares and sums are float64
 * (a float32 sum of squares overflows at |g| ~ 1.8e19 and flushes squares below 1e-38), folded per thread in index order and
 * then by a fixed tree over the workgroup into ONE float64 partial in the workspace.  The second is one workgroup that folds
 * the partials the same way (thread t takes partials t, t + 256, ... in index order, then the same tree) and writes `out`.
 * No floating-point atomics, no completion counters: the work split depends on n only and two calls on the same data give the
 * same bits.  NaN and Inf reach out[0]: a NaN anywhere makes it NaN (the max keeps a NaN on either side, as torch.maximum),
 * +-Inf makes it +Inf.  n == 0: one launch, out = {0, 1}; the workspace may be NULL then.
 * workspace: ebfi_grad_norm_workspace(n) bytes = 8 ceil(n / EBFI_GRAD_NORM_CHUNK) (host arithmetic; 0 for n <= 0), 16-byte
 * aligned, overwritten by every call.  No allocation, no synchronisation: capturable.
 * Null grad (n > 0) / out, n < 0, an unknown norm_kind, max_norm not positive (or NaN), misaligned grad or workspace ->
 * EBFI_ERR_ARG; a missing or short workspace -> EBFI_ERR_WORKSPACE; a grid beyond 2^31 - 1 -> EBFI_ERR_UNSUPPORTED; none of them
 * touches the GPU. */
#define EBFI_NORM_L2 0
#define EBFI_NORM_INF 1
#define EBFI_GRAD_NORM_CHUNK 16384
int64_t ebfi_grad_norm_workspace(int64_t n);
int ebfi_grad_norm(const float *grad, int64_t n, int norm_kind, double max_norm, float *out, void *workspace,
                   int64_t workspace_bytes, void *stream);

/* ebfi_optim_step with a gradient scale and an exponential moving average of the parameters folded into the SAME launch.
 * Arguments up to `flag` as in ebfi_optim_step.  With grad_scale == NULL and ema == NULL the call IS ebfi_optim_step (forwarded
 * unchanged: the same kernels, the same bits).  Otherwise ONE launch of the spelled-out law of ebfi_optim_step's variants,
 * operation by operation, contraction off -- plain Adam (no weight decay, no AMSGrad) included, which here runs that law
 * instead of the kernel of ebfi_adam_step:
 *   g' = g * grad_scale[0]          first: before the L2 weight-decay fma, as clipping precedes the optimiser in torch.
 *                                   grad_scale: one device float (out + 1 of ebfi_grad_norm), NULL = no scale.  `grad` is only
 *                                   read, the scaled gradient is never written anywhere.
 *   the update of ebfi_optim_step on g' -> p_new
 *   e <- e + w (p_new - e)          ema float32 [n], 16-byte aligned, NULL = none; w = (float)(1 - d) with d = ema_decay, or
 *                                   min(ema_decay, (1 + t) / (10 + t)) when ema_warmup != 0; t = ema_step[0] in double.
 * ema_step: one device float holding the ALREADY incremented count of applied averages (the host increments it before the
 * launch), required with ema.  guard / flag: the protocol of ebfi_optim_step, extended: a skipped step writes no parameter, no
 * state and no ema element, takes BOTH step words back and counts ONCE in guard[1].
 * Errors as ebfi_optim_step; ema without ema_step, a misaligned ema, ema_decay outside [0, 1) -> EBFI_ERR_ARG.
 * Bytes moved per launch: those of ebfi_optim_step + 8 n with ema. */
int ebfi_optim_step_ex(int kind, int flags, float *param, const float *grad, float *state0, float *state1, float *state2,
                       float *step, int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                       double momentum, double dampening, int *guard, const float *flag, const float *grad_scale, float *ema,
                       float *ema_step, double ema_decay, int ema_warmup, void *stream);

/* Gradient packing of a training step (replaces the bucket copy of DistributedDataParallel, train_ours.py:754, and the
 * 255-piece concatenation of earlier rounds): `grads` / `numels` are HOST arrays of `count` device pointers (NULL: that
 * parameter has no gradient, its range is zero-filled) and element counts (sum = total); tensor k is copied to
 * flat[sum of numels[0..k-1] ...].  Then flat[total] = (guard && guard[0] != 0) ? 1 : 0 and flat[total + 1 .. total + pad - 1]
 * = 0 (1 <= pad <= 256: the wire buffer's trailer).  The pointers travel by value in the kernel arguments, 128 per launch:
 * a captured launch replays with the addresses the capture saw (graph-pool allocations keep them). */
int ebfi_grad_gather(const void *const *grads, const int64_t *numels, int count, float *flat, int64_t total, int pad,
                     const int *guard, void *stream);


/* ------------------------------------------------------------------ evaluation metrics
 * Per frame n of an fp32 pair pred / target [N, C, H, W] (the evaluation loop's psnr_loss / ssim_loss / nn.MSELoss,
 * loss/restore.py:43-92, one reference call per frame):
 *   ssim[n] = mean over c of the mean over the interior pixels [3, H-3) x [3, W-3) of the SSIM map of scikit-image's
 *             structural_similarity defaults: 7x7 uniform window, sample covariance (x 49/48), C1 = (0.01 R)^2, C2 = (0.03 R)^2,
 *             R = ssim_data_range (2 reproduces the reference's float32 call without data_range)
 *   psnr[n] = C >= 2: mean over c of 10 log10(dr_c^2 / mse_c), mse_c = mean((target_c - pred_c)^2) unclipped,
 *             dr_c = max(target_c) - min(target over all channels) (the reference's data range);
 *             C == 1: 10 log10(1 / mse) of both images clipped to [0, 1]
 *   mse[n]  = mean((pred - target)^2) over C*H*W
 * A non-finite value anywhere in frame n's pred or target makes its three outputs NaN; mse_c = 0 gives +inf.
 * Strides (elements, any int64) of N, C and rows; the column stride must be 1 (EBFI_ERR_UNSUPPORTED otherwise).  16-byte row
 * loads when both base pointers are 16-byte aligned and all strides are multiples of 4, scalar loads otherwise.
 * Two launches on `stream` (per-tile partials into `workspace`, then a fixed-order fp64 reduction per frame): no host
 * synchronisation, no allocation, no atomics -- capturable, and bit-reproducible.  workspace: 16-byte aligned, at least
 * ebfi_image_metrics_workspace(N, C, H, W) bytes (pure host arithmetic; 0 for a bad shape).  out_*: device float[N].
 * Null pointers, C < 1, H < 7 or W < 7 (scikit-image refuses a window larger than the image) or a ssim_data_range that is
 * not positive -> EBFI_ERR_ARG; a short workspace -> EBFI_ERR_WORKSPACE; neither touches the GPU. */
int64_t ebfi_image_metrics_workspace(int64_t N, int C, int H, int W);
int ebfi_image_metrics(const float *pred, const int64_t pred_strides[4], const float *target, const int64_t target_strides[4],
                       int64_t N, int C, int H, int W, float ssim_data_range, void *workspace, int64_t workspace_bytes,
                       float *out_psnr, float *out_ssim, float *out_mse, void *stream);

/* ------------------------------------------------------------------ evaluation LPIPS (AlexNet, v0.1)
 * Per pair n of an fp32 pred / target [N, C, H, W] (the evaluation loop's perceptual_loss(net='alex'), eval mode, spatial=False):
 *   x'       = ((2x - 1) - shift_c) / scale_c with normalize != 0, (x - shift_c) / scale_c otherwise;
 *              shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450); zero padding applies after it
 *   f1 .. f5 = the five ReLU outputs of AlexNet's `features`: conv1 11x11/s4/p2 3->64, maxpool 3/s2, conv2 5x5/p2 64->192,
 *              maxpool 3/s2, conv3 3x3/p1 192->384, conv4 3x3/p1 384->256, conv5 3x3/p1 256->256 (pools: no padding, floor
 *              mode, NaN propagating)
 *   d_l(p)   = sum_c w_lc (u0_c - u1_c)^2,  u = f / (sqrt(sum_c f_c^2) + 1e-10) of pred (u0) and target (u1)
 *   lpips[n] = sum_l mean_p d_l(p);  out_layers[n][l] = mean_p d_l(p) (the reference's retPerLayer; may be NULL)
 * C == 1 is read as three equal channels.  The convolutions run on exact fp32 MFMA; the per-pixel distances are summed in fp64
 * in a fixed order.  A NaN or Inf anywhere in pair n's pred or target makes lpips[n] and its layers NaN, no other pair.
 * Strides (elements, any int64) of N, C and rows; the column stride must be 1.
 * ebfi_lpips_pack_params packs the five conv weights [Cout][Cin][k][k], biases [Cout] and head vectors [Cout] (the 1x1 heads
 * lin{l}.model.1.weight) -- host arrays of 5 device pointers each, fp32 contiguous -- into `params` (16-byte aligned, at least
 * ebfi_lpips_params_bytes() bytes), on `stream`.  workspace: 16-byte aligned, at least ebfi_lpips_workspace(N, C, H, W) bytes
 * (pure host arithmetic; 0 for a bad shape): the five ReLU maps of all 2N images, tile partials and non-finite flags.
 * Launches on `stream` only: no host synchronisation, no allocation, no atomics -- capturable, and bit-reproducible.
 * Null pointers, C not in {1, 3}, H or W < 31 (AlexNet's trunk needs 31), a column stride other than 1 -> EBFI_ERR_ARG; a short
 * workspace or params buffer -> EBFI_ERR_WORKSPACE; neither touches the GPU. */
int64_t ebfi_lpips_params_bytes(void);
int ebfi_lpips_pack_params(const float *const *conv_w, const float *const *conv_b, const float *const *lin_w, void *params,
                           int64_t params_bytes, void *stream);
int64_t ebfi_lpips_workspace(int64_t N, int C, int H, int W);
int ebfi_lpips_alex(const float *pred, const int64_t pred_strides[4], const float *target, const int64_t target_strides[4],
                    int64_t N, int C, int H, int W, int normalize, const void *params, void *workspace, int64_t workspace_bytes,
                    float *out_lpips, float *out_layers, void *stream);

/* ------------------------------------------------------------------ evaluation LPIPS (VGG-16, v0.1)
 * perceptual_loss(net='vgg'): the definition of ebfi_lpips_alex with the trunk exchanged (PNetLin(pnet_type='vgg', version='0.1',
 * spatial=False) in eval mode).  x', d_l, lpips[n], out_layers, the strides, the NaN / Inf rule and the launch contract are those
 * above; the zero padding of the first convolution applies to x' (it is not folded into the weights).
 *   f1 .. f5 = the ReLU outputs of conv1_2, conv2_2, conv3_3, conv4_3, conv5_3 (64, 128, 256, 512, 512 channels) of torchvision's
 *              vgg16.features: 13 convolutions 3x3 / stride 1 / pad 1 with bias and ReLU, channels
 *              3-64-64 | 128-128 | 256-256-256 | 512-512-512 | 512-512-512, `|` a 2x2 / stride 2 max-pool without padding in floor
 *              mode (an odd last row or column is dropped; NaN propagating)
 * The convolutions are ebfi_conv2d_forward's exact-fp32 3x3 kernel, called inside; each tap map is read by one kernel that
 * forms the norms and the head-weighted differences in fp64 and writes the pooled map of the next block.
 * ebfi_lpips_vgg_pack_params takes host arrays of 13 (conv_w [Cout][Cin][3][3], conv_b [Cout], in the order of the keys
 * features.{0,2,5,7,10,12,14,17,19,21,24,26,28}) and 5 (lin_w) device pointers, fp32 contiguous.  workspace: the scaled inputs,
 * two maps of the largest layer ([2N][64][H][W] fp32 each: 0.94 GB per 720 x 1280 pair together), tile partials and flags.
 * H, W >= 16 (four pools must leave a pixel); H * W <= 4063231 and N <= 16384 in one call; ebfi_lpips_vgg_workspace returns 0
 * for a shape the entry point refuses.  Error codes as ebfi_lpips_alex. */
int64_t ebfi_lpips_vgg_params_bytes(void);
int ebfi_lpips_vgg_pack_params(const float *const *conv_w, const float *const *conv_b, const float *const *lin_w, void *params,
                               int64_t params_bytes, void *stream);
int64_t ebfi_lpips_vgg_workspace(int64_t N, int C, int H, int W);
int ebfi_lpips_vgg(const float *pred, const int64_t pred_strides[4], const float *target, const int64_t target_strides[4],
                   int64_t N, int C, int H, int W, int normalize, const void *params, void *workspace, int64_t workspace_bytes,
                   float *out_lpips, float *out_layers, void *stream);

/* ------------------------------------------------------------------ LPIPS (VGG-16, v0.1) as a training loss
 * The reference's perceptual_loss is a loss (train_ours.py:765 builds it with its default trunk, net='alex'; this is the same loss
 * with net='vgg'): autograd carries it into the prediction.  Here
 * ebfi_lpips_vgg_forward_train takes the arguments of ebfi_lpips_vgg and writes the same out_lpips / out_layers, bit for bit
 * (the same kernels on the same values in the same order of sums: each image's convolution tiles do not depend on the batch they
 * are launched in), and keeps in `workspace` (at least ebfi_lpips_vgg_train_workspace(N, C, H, W) bytes, pure host arithmetic, 0
 * for a shape ebfi_lpips_vgg refuses) what the backward needs: the 13 ReLU outputs of the pred images, the 5 tap maps of the
 * target images and the non-finite flags, beside two maps [N][64][H][W] the target's other layers and then the gradients
 * alternate between.  (2.00 GB per 720 x 1280 pair, 1.14 GB for 8 pairs of 256 x 256.)
 *
 * ebfi_lpips_vgg_backward reads that workspace (of the forward_train call with the same N, C, H, W, normalize and params; it
 * writes the gradient maps into it, so one backward per forward) and grad_out, device float[N], the gradient with respect to
 * lpips[n], and fully overwrites grad_pred [N, C, H, W] fp32 through grad_pred_strides (elements; column stride 1).  The target
 * gets no gradient.  Per pair n, tap layer l of size H_l x W_l and pixel p, with x = f0(p) the pred features, y = f1(p) the
 * target's:
 *   n0 = sqrt(sum_c x_c^2), r0 = 1 / (n0 + 1e-10); n1, r1 likewise of y
 *   a_c = 2 w_c (r0 x_c - r1 y_c)
 *   S = sum_c a_c x_c = 2 (r0 sum_c w_c x_c^2 - r1 sum_c w_c x_c y_c)
 *   dL/dx_k = grad_out[n] / (H_l W_l) * (a_k r0 - x_k r0^2 S / n0);  exactly 0 for every k where n0 == 0
 * (at n0 == 0 every x_k is a ReLU zero, which the mask of the convolution's data gradient removes in torch as well; the kernel
 * writes the zero itself, because that mask is a product and 0 * NaN is NaN).  The sums are formed in fp64 from the fp32 maps.
 * One fused kernel per tap layer mirrors the forward's: it adds to dL/dx the gradient of the pooled map that the next block
 * returned (none for f5), routed to the first maximum of each 2x2 window in row-major order (torch's rule; the last row / column
 * of an odd map gets a tap gradient and no routed one), and writes the sum for the pred images.  The 13 data gradients are
 * ebfi_conv2d_backward_data (EBFI_F32, act = 1 at slope 0: the ReLU mask read from the saved output) between the two gradient
 * maps, pred images only.  Input epilogue, with mul_c = (normalize ? 2 : 1) / scale_c: grad_pred[n, c] = mul_c * grad_x'[n, c]
 * for C == 3, the sum over the three c for C == 1.  A pair whose pred or target held a NaN or Inf (the forward's flags) gets
 * grad_pred[n] NaN everywhere; no other pair is touched by it.
 * Both follow the launch contract of ebfi_lpips_alex (on `stream` only, no host synchronisation, no allocation, no atomics:
 * capturable and bit-reproducible) and its error codes; argument errors touch no GPU.  The AlexNet trunk's training form is the
 * next section. */
int64_t ebfi_lpips_vgg_train_workspace(int64_t N, int C, int H, int W);
int ebfi_lpips_vgg_forward_train(const float *pred, const int64_t pred_strides[4], const float *target,
                                 const int64_t target_strides[4], int64_t N, int C, int H, int W, int normalize, const void *params,
                                 void *workspace, int64_t workspace_bytes, float *out_lpips, float *out_layers, void *stream);
int ebfi_lpips_vgg_backward(const float *grad_out, const void *params, void *workspace, int64_t workspace_bytes, int64_t N, int C,
                            int H, int W, int normalize, float *grad_pred, const int64_t grad_pred_strides[4], void *stream);

/* ------------------------------------------------------------------ LPIPS (AlexNet, v0.1) as a training loss
 * The trunk the reference trains with: its trainer builds perceptual_loss(gpu_ids=[local_rank]) (train_ours.py:765), and 'alex'
 * is the default net of loss/restore.py:12.  ebfi_lpips_alex_forward_train takes the arguments of ebfi_lpips_alex and writes the
 * same out_lpips / out_layers, bit for bit: it launches the same kernels on the same values, and the front of its workspace (at
 * least ebfi_lpips_alex_train_workspace(N, C, H, W) bytes, pure host arithmetic, 0 for a shape ebfi_lpips_alex refuses) is the
 * score's workspace -- f1 .. f5 of all 2N images, the tile partials and the non-finite flags -- followed by the two gradient
 * maps of the pred images that the backward alternates between (each as large as the largest of f1 .. f5 of N images).
 * (57.2 MB for 8 pairs of 256 x 256, 105.1 MB for one 720 x 1280 pair: the score's 41.0 / 75.9 MB and the two maps.)
 *
 * ebfi_lpips_alex_backward reads that workspace (of the forward_train call with the same N, C, H, W, normalize and params; it
 * writes the gradient maps into it, so one backward per forward) and grad_out, device float[N], and fully overwrites grad_pred
 * [N, C, H, W] fp32 through grad_pred_strides (elements; column stride 1).  The target gets no gradient.  The gradient's
 * definition is that of ebfi_lpips_vgg_backward above -- n0, r0, a_c, S, dL/dx_k, exactly 0 where n0 == 0, the sums in fp64 from
 * the fp32 maps -- with AlexNet's trunk around it.  Launches, pred images only:
 *   tap adjoint x5    sixteen threads per pixel of a tap map: the distance gradient, plus the gradient that arrives from the next
 *                     block.  For f3 and f4 that is a map of the same size; for f1 and f2 it is the gradient of the 3x3 / stride 2
 *                     pooled map, gathered: a pixel lies in at most 2 x 2 windows, and a window's gradient is added if and only if
 *                     the pixel is the window's first maximum in row-major order (torch's rule), found again from the kept map --
 *                     no pooled map and no argmax is stored, and no atomics are used.  Rows and columns past the last window get
 *                     a tap gradient and no routed one.
 *   conv5 .. conv2    one kernel of lpips.hip, an implicit GEMM on exact fp32 MFMA (v_mfma_f32_32x32x2_f32) with the taps
 *                     flipped: K = 256 x 9, 256 x 9, 384 x 9 and, for the 5x5 layer, 192 x 25; the gradient patch of an 8 x 8 tile
 *                     staged in LDS as the forward stages its input, the ReLU mask of the kept output applied on the way
 *   conv1 (11x11/s4)  a direct fp32 kernel in a fixed order of sums: input row i = 4 q + r - 2 takes the taps k = 4 d + r of the
 *                     output rows q - d, d in {0, 1, 2}, so a thread keeps the 3 x 3 x 3 weights of one phase (r_y, r_x) and
 *                     one output channel in registers for four pixels.  Its epilogue is the input epilogue: with mul_c =
 *                     (normalize ? 2 : 1) / scale_c, grad_pred[n, c] = mul_c * grad_x'[n, c] for C == 3, the sum over the three c
 *                     for C == 1.  An input row or column that no conv1 window covers (row 33 of a 34-row image) gets exactly 0.
 * A pair whose pred or target held a NaN or Inf (the forward's flags) gets grad_pred[n] NaN everywhere; no other pair is touched
 * by it.  Exact fp32 in the convolutions, fp64 in the tap sums; no bf16 or fp16 operand.
 * grad_params (16-byte aligned, at least ebfi_lpips_alex_grad_params_bytes() bytes) holds the five conv weights in the layouts
 * the data gradients stage from -- conv1 as given ([64][3][11][11]), conv2 .. conv5 as the flipped implicit-GEMM image
 * [Cout][k][k][Cin] -- packed once by ebfi_lpips_alex_pack_grad_params from a host array of 5 device pointers (the
 * conv_w of ebfi_lpips_pack_params).  `params` stays what ebfi_lpips_pack_params wrote: its size and bits do not change.
 * The launch contract is ebfi_lpips_alex's (on `stream` only, no host synchronisation, no allocation, no atomics: capturable and
 * bit-reproducible), and so are the shape limits (H, W >= 31) and the error codes; argument errors touch no GPU. */
int64_t ebfi_lpips_alex_grad_params_bytes(void);
int ebfi_lpips_alex_pack_grad_params(const float *const *conv_w, void *grad_params, int64_t bytes, void *stream);
int64_t ebfi_lpips_alex_train_workspace(int64_t N, int C, int H, int W);
int ebfi_lpips_alex_forward_train(const float *pred, const int64_t pred_strides[4], const float *target,
                                  const int64_t target_strides[4], int64_t N, int C, int H, int W, int normalize, const void *params,
                                  void *workspace, int64_t workspace_bytes, float *out_lpips, float *out_layers, void *stream);
int ebfi_lpips_alex_backward(const float *grad_out, const void *params, const void *grad_params, void *workspace,
                             int64_t workspace_bytes, int64_t N, int C, int H, int W, int normalize, float *grad_pred,
                             const int64_t grad_pred_strides[4], void *stream);

/* ------------------------------------------------------------------ Charbonnier loss (validation)
 * CharbonnierLoss of the reference (loss/restore.py:95-105; the validation score of train_ours.py:588) per sample n of an fp32
 * pair x / y [N, C, H, W]:
 *   out[n] = sum over c, h, w of sqrt((x - y)^2 + eps)        -- a SUM, not a mean; eps sits under the root and is not squared
 * (the reference's scalar is the sum of out over n).  Every term is formed in fp32 (subtract, fused multiply-add, root) and
 * accumulated in fp64; out[n] is rounded to fp32 once.  A NaN or inf element makes out[n] non-finite: nothing is dropped.
 * Strides (elements, any int64) of N, C and rows; the column stride must be 1 (EBFI_ERR_UNSUPPORTED otherwise).  16-byte loads
 * when both base pointers are 16-byte aligned and all strides are multiples of 4, scalar loads otherwise.
 * Forward: two launches on `stream` (one fp64 partial per tile into `workspace`, then a fixed-order fp64 reduction per sample):
 * no host synchronisation, no allocation, no atomics -- capturable, and bit-reproducible.  A tile is R = ceil(4096 / W)
 * consecutive rows of a sample's C * H rows; workspace: 16-byte aligned, at least ebfi_charbonnier_workspace(N, C, H, W) =
 * N * ceil(C * H / R) * 8 bytes (pure host arithmetic; 0 for a bad shape).  out: device float[N].
 * Backward: grad_x[n,c,h,w] = g[0] * (x - y) / sqrt((x - y)^2 + eps), g a device scalar (the gradient with respect to y is
 * its negative), written to a CONTIGUOUS [N, C, H, W] tensor in one streaming launch.
 * Null pointers, N < 0, C / H / W < 1, eps not positive and finite, a misaligned workspace -> EBFI_ERR_ARG; a column stride
 * other than 1 -> EBFI_ERR_UNSUPPORTED; a short workspace -> EBFI_ERR_WORKSPACE; none of them touches the GPU. */
int64_t ebfi_charbonnier_workspace(int64_t N, int C, int H, int W);
int ebfi_charbonnier_forward(const float *x, const int64_t x_strides[4], const float *y, const int64_t y_strides[4], int64_t N,
                             int C, int H, int W, float eps, void *workspace, int64_t workspace_bytes, float *out, void *stream);
int ebfi_charbonnier_backward(const float *x, const int64_t x_strides[4], const float *y, const int64_t y_strides[4], int64_t N,
                              int C, int H, int W, float eps, const float *g, float *grad_x, void *stream);

/* ------------------------------------------------------------------ duty head + MSE loss (stage-1 pre-training)
 * The tail of ExposureDecision.forward (reference models/Ours/model_singleframe.py:75-76) and the loss of
 * train_ours_exposuredecision.py:250-252 for an fp32 map ex [B, 1, H, W]:
 *   Ex[b] = sigmoid(mean over h, w of ex[b, 0, h, w])
 *   loss  = scale * mean over b of (Ex[b] - duty[b])^2        -- MSELoss(Ex, duty) / accu_step with scale = 1 / accu_step
 * The plane sum is accumulated in fp64 from the fp32 elements, mean and sigmoid are formed in fp64 and Ex[b] is rounded to
 * fp32 once; the loss is summed in fp64 over the ROUNDED Ex (what backward reads) and rounded once.  A NaN or inf element
 * reaches its own sample's Ex and the loss, no other sample's Ex: nothing is masked.  duty == NULL: Ex only (loss_out unused).
 * ex_strides (elements, any int64) of B, the single channel (ignored) and rows; the column stride must be 1
 * (EBFI_ERR_UNSUPPORTED otherwise).  16-byte loads when the base pointer is 16-byte aligned and both strides are multiples
 * of 4, scalar loads otherwise and for a ragged row tail.
 * Forward: two launches on `stream` (one fp64 partial per tile of R = ceil(4096 / W) rows into `workspace`, then ONE workgroup
 * that reduces in a fixed order): no host synchronisation, no allocation, no atomics -- capturable, and bit-reproducible.
 * workspace: 16-byte aligned, at least ebfi_duty_head_workspace(B, H, W) = B * ceil(H / R) * 8 bytes (pure host arithmetic; 0
 * for a bad shape).  duty: device float[B]; Ex_out: device float[B]; loss_out: device float[1].
 * Backward: grad_ex[b, :, :] = g[0] * scale * 2 (Ex[b] - duty[b]) / B * Ex[b] (1 - Ex[b]) / (H * W), g a device scalar, one
 * streaming fill of a CONTIGUOUS [B, 1, H, W] tensor; a plane is constant bit for bit.
 * Null pointers (other than duty in forward), B < 0, H / W < 1, a non-finite scale, a misaligned workspace -> EBFI_ERR_ARG;
 * a short workspace -> EBFI_ERR_WORKSPACE; none of them touches the GPU. */
int64_t ebfi_duty_head_workspace(int64_t B, int H, int W);
int ebfi_duty_head_forward(const float *ex, const int64_t ex_strides[4], const float *duty, int64_t B, int H, int W, float scale,
                           void *workspace, int64_t workspace_bytes, float *Ex_out, float *loss_out, void *stream);
int ebfi_duty_head_backward(const float *g, const float *Ex, const float *duty, int64_t B, int H, int W, float scale,
                            float *grad_ex, void *stream);

/* ------------------------------------------------------------------ frame I/O of an inference run on recorded clips
 * ebfi_frames_u8_to_planar: n stored frames, interleaved uint8 (pixel (f, Y, X) at src + f * src_strides[0] + Y * src_strides[1]
 * + X * src_strides[2], its three channels adjacent; frames of H0 x W0 pixels) -> out float32 [n][3][h][w], contiguous:
 *   out[f][c][y][x] = (float) src[f][i + (flip_v ? h-1-y : y)][j + (flip_h ? w-1-x : x)][reverse_channels ? 2-c : c] / 255.0f
 * i.e. `torch.from_numpy(frames).permute(0, 3, 1, 2).float() / 255` (dataloader/h5dataset_realdata.py:189) of the window
 * (i, j, h, w), bit for bit (one correctly rounded fp32 division), with the crop and the flips of AugmentData folded into the
 * read.  reverse_channels: the BGR -> RGB swap of the synthetic-blur reader (h5dataset.py:296-311); the real-data reader does
 * not swap.
 * ebfi_planar_to_u8: in float32 (pixel (f, c, y, x) at in + f * in_strides[0] + c * in_strides[1] + y * in_strides[2] + x)
 * -> out uint8 [n][H][W][3], contiguous:
 *   out[f][y][x][c] = (uint8) trunc(min(max(in[f][c][y][x], 0), 1) * 255.0f)
 * i.e. `(x.clamp(0, 1) * 255).cpu().numpy().transpose(0, 2, 3, 1).astype('uint8')` (infer_ours.py:135) for every finite and
 * infinite input, bit for bit.  NaN gives 0 (numpy leaves that cast undefined).
 * Strides in ELEMENTS, int64, >= 0 (the pixel stride of `src` >= 3).  One thread moves four pixels of a row in all three
 * channels.  The planar side uses 16-byte accesses when its base pointer is 16-byte aligned and the width (and, for `in`, every
 * stride) is a multiple of 4; the interleaved side uses 4-byte accesses when its base pointer is 4-byte aligned (and, for
 * `src`, the frame and row strides and j are multiples of 4 and the pixel stride is 3).  Anything else -- a ragged width, a
 * view that starts mid-row, a byte-offset source -- runs a scalar path with no alignment requirement: the entry point decides
 * from the actual pointers, nothing is assumed.  One launch on `stream`, no workspace, no host synchronisation: capturable.
 * Null pointers, n < 0, sizes < 1, a window that leaves the frame, a negative stride -> EBFI_ERR_ARG before anything touches
 * the GPU; n == 0 is a no-op. */
int ebfi_frames_u8_to_planar(const uint8_t *src, const int64_t src_strides[3], int64_t n, int H0, int W0, int i, int j, int h,
                             int w, int reverse_channels, int flip_h, int flip_v, float *out, void *stream);
int ebfi_planar_to_u8(const float *in, const int64_t in_strides[3], int64_t n, int H, int W, uint8_t *out, void *stream);

/* ebfi_period_frames_u8: one period of a TRAINING item (the synthetic-blur reader, dataloader/h5dataset.py:296-311) in one pass
 * over its n stored frames.  Source layout, window, channel reversal and flips are those of ebfi_frames_u8_to_planar;
 *   sharp float32 [n][3][h][w], contiguous: sharp[f] is what ebfi_frames_u8_to_planar writes for frame f;
 *   blur  float32 [3][h][w], contiguous: the mean of the first n_blur frames of the same window,
 *     blur[c][y][x] = (float) ((double) (sum over f < n_blur of the byte) / (double) n_blur) / 255.0f
 * i.e. `torch.from_numpy(FNumpy[:n_blur].mean(0)).permute(2, 0, 1).float() / 255` (h5dataset.py:311), bit for bit: the byte sum
 * is an exact integer, numpy's mean divides it in float64, the quotient is rounded to fp32 and divided by 255 in fp32 -- three
 * roundings, made here in the same places (a fused sum / (255 * n_blur) gives other bits).  Every source byte is read once.
 * `sharp` and `blur` may point into larger tensors (a slot of a batch): 16-byte stores are used when w % 4 == 0 and BOTH
 * pointers are 16-byte aligned, 4-byte loads under the conditions of ebfi_frames_u8_to_planar, the scalar path otherwise.
 * One thread owns four pixels of a row and walks the frames.  One launch on `stream`, no workspace, no host synchronisation.
 * Null pointers, n < 1, n_blur < 1, n_blur > n (or > 2^24), sizes < 1, a window that leaves the frame, a negative stride (pixel
 * stride < 3) -> EBFI_ERR_ARG before anything touches the GPU. */
int ebfi_period_frames_u8(const uint8_t *src, const int64_t src_strides[3], int64_t n, int64_t n_blur, int H0, int W0, int i,
                          int j, int h, int w, int reverse_channels, int flip_h, int flip_v, float *sharp, float *blur,
                          void *stream);

/* ------------------------------------------------------------------ event augmentation of the clip loaders, device law
 * The device-native counterpart of AugmentData's crop / flips / add_noise / add_hot_pixels on an event stack
 * (dataloader/h5dataset.py:368-463).  The random law is integer-only, so a host restatement gives the same bits:
 *   generator  Philox4x32-10, key = (seed low word, seed high word), counter = (g low, g high, stream, 0), four words per call;
 *   count      a draw of one word u gives k = #{m : u < table[m]}, table[m] = floor(2^32 f erfc((m + 1) / (std sqrt 2))) made
 *              on the HOST, strictly decreasing, at most EBFI_NOISE_TABLE_MAX entries: the distribution of int(|N(0, std)|)
 *              on a fraction f of the draws.  No transcendental runs on the device.
 *
 * ebfi_event_augment: source float32 [TB][2][H0][W0] (value (b, p, Y, X) at src + b * src_strides[0] + p * src_strides[1] +
 * Y * src_strides[2] + X: a transposed view is read in place) -> dst float32 [TB][2][h][w], contiguous:
 *   dst[b][p][y][x] = src[b][p][i + (flip_v ? h-1-y : y)][j + (flip_h ? w-1-x : x)] + k(cell)
 * where cell = cell_offset + the linear index in dst and k(cell) is the count drawn from word (cell & 3) of Philox group
 * (cell >> 2) of stream 0.  cell_offset is 0 for an item made in one call; an item of several loads passes each load's first
 * cell.  table_len == 0: no noise (k = 0), `table` may then be null.  A thread owns four consecutive cells of dst: one
 * 16-byte store when dst is 16-byte aligned; one 16-byte load when its four cells lie in one row and their source address is
 * 16-byte aligned (mirrored in registers under flip_h), scalar loads otherwise; the last cells of a stack whose size is no
 * multiple of 4 are stored one by one.  Cell indices are 64-bit.  One launch on `stream`, no workspace, no synchronisation.
 * Null pointers, TB < 1, sizes < 1, a window that leaves the frame, h * w >= 2^31, a negative stride, a negative cell_offset,
 * table_len outside [0, EBFI_NOISE_TABLE_MAX], source and destination ranges that overlap -> EBFI_ERR_ARG, nothing launched.
 *
 * ebfi_event_hot_pixels: in place on stack float32 [planes][h][w], contiguous.  Hot pixel n < n_hot takes words u0, u1, u2 of
 * group n of stream 1: x = (u0 * w) >> 32, y = (u1 * h) >> 32, amplitude k from u2 through `table` (made with f = 1); k is
 * added to every plane at (y, x), repeated positions accumulate.  The adds are float atomics of integers: exact and
 * order-free while every sum stays below 2^24, so the result does not depend on the launch geometry.  n_hot == 0 or
 * table_len == 0 is a no-op.  Null stack, sizes < 1, h * w >= 2^31, n_hot < 0 or planes * n_hot >= 2^40, table_len outside
 * [0, EBFI_NOISE_TABLE_MAX] -> EBFI_ERR_ARG. */
#define EBFI_NOISE_TABLE_MAX 32
int ebfi_event_augment(const float *src, const int64_t src_strides[3], int64_t TB, int H0, int W0, int i, int j, int h, int w,
                       int flip_h, int flip_v, uint64_t seed, const uint32_t *table, int table_len, int64_t cell_offset,
                       float *dst, void *stream);
int ebfi_event_hot_pixels(float *stack, int64_t planes, int h, int w, uint64_t seed, const uint32_t *table, int table_len,
                          int64_t n_hot, void *stream);

/* ------------------------------------------------------------------ event-count images of the evaluation loop
 * ebfi_event_cnt_image: n images of two polarity planes, float32 (value (f, p, y, x) at ev + f * ev_strides[0] + p * ev_strides[1]
 * + y * ev_strides[2] + x; p = 0 positive, 1 negative) -> out uint8 [n][H][W][3], contiguous: for every image what
 *   event_visualisation().plot_event_cnt(ev[f].transpose(1, 2, 0), False, color_scheme=..., use_opencv=..., is_black_background=...,
 *                                        is_norm=...)
 * returns (myutils/vis_events/matplotlib_plot_events.py:127-251; infer_ours.py:139-142 calls it once per time bin of a load with
 * SeqHREv[0], 'blue_red', a white background and normalisation), bit for bit for every finite float32 input: negative values,
 * denormals and values spanning many exponents included, not only counts.
 * With is_norm the planes are normalised by np.percentile(plane, 1) and np.percentile(plane, 99) of both polarities.  Each
 * percentile interpolates two adjacent order statistics; the four per plane are found exactly by a three-pass (11 + 11 + 10 bit)
 * radix select over an order-preserving integer key of the float, with integer histograms in LDS merged by integer adds, so the
 * result does not depend on arrival order; the ranks and weights (numpy's 'linear' method as it behaves for a float32 array)
 * are host arithmetic from H * W, and one device thread per plane interpolates in numpy's operation order.  Without is_norm
 * no percentile is needed and none is computed: one launch.  The colour map follows the reference's evaluation order and
 * types (fp32 normalisation with one correctly rounded division, clip, masks, `1 - x` in fp32, `* 255` and the truncating cast
 * in double); the reference's final BGR -> RGB reversal is folded into the store and omitted when use_opencv is set.
 * color_scheme: EBFI_EVENT_BLUE_RED or EBFI_EVENT_GREEN_RED.  EBFI_EVENT_GRAY -> EBFI_ERR_UNSUPPORTED: in the reference it only
 * runs with use_opencv=True (cv2.cvtColor refuses its two-dimensional canvas otherwise) and nothing calls it.
 * Strides in ELEMENTS, int64, >= 0; the column stride is 1.  16-byte loads when W % 4 == 0, `ev` is 16-byte aligned and every
 * stride is a multiple of 4, dword stores when `out` is 4-byte aligned as well; anything else runs a scalar path with no
 * alignment requirement, decided from the actual pointers and strides.
 * workspace: ebfi_event_cnt_image_workspace(n, H, W, is_norm) bytes (pure host arithmetic; 0 without is_norm, for n == 0 and
 * for a bad shape), 16-byte aligned, overwritten by every call.  A memset, six small-to-streaming launches and the colour map
 * go onto `stream` with no host synchronisation between them: capturable.
 * Null pointers, n < 0, H or W < 1, a negative stride, an unknown scheme, a misaligned workspace -> EBFI_ERR_ARG; a missing or
 * short workspace -> EBFI_ERR_WORKSPACE; H * W or the launch grid beyond 2^31 - 1 -> EBFI_ERR_UNSUPPORTED; none of them touches
 * the GPU.  n == 0 is a no-op. */
enum { EBFI_EVENT_BLUE_RED = 0, EBFI_EVENT_GREEN_RED = 1, EBFI_EVENT_GRAY = 2 };
int64_t ebfi_event_cnt_image_workspace(int64_t n, int H, int W, int is_norm);
int ebfi_event_cnt_image(const float *ev, const int64_t ev_strides[3], int64_t n, int H, int W, int color_scheme,
                         int is_black_background, int is_norm, int use_opencv, uint8_t *out, void *workspace,
                         int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ per-segment statistics of a flat buffer (training monitor)
 * ebfi_segment_stats: x float32 [n]; offsets int64 [S + 1] ON THE DEVICE (segment s = x[offsets[s] .. offsets[s + 1]); the entry
 * point never reads them, the kernels clamp them into [0, n] and make them ascending, so no table can take a load out of
 * bounds); limits float64 [nb] on the device, ascending.  For every segment:
 *   moments[s] = {finite count, non-finite count, min, max, sum, sum of squares}   float64 [S][6], over the FINITE values
 *   hist[s][i] = number of finite values v with limits[i - 1] < v <= limits[i]      int32 [S][nb]; bucket 0 starts at -inf, a
 *                value above the last limit counts in the last bucket
 * NaN and +-Inf count in the non-finite column only.  An empty segment gives counts 0, min +inf, max -inf, sums 0.  Every
 * value is widened to float64 first: comparisons, sums and squares are float64; the limits table is staged in LDS and searched
 * by bisection (no log / pow); counts are integer adds (LDS, then global).  Sums are folded in one fixed order (per thread in
 * index order, a fixed tree over the workgroup, a fixed fold over the segment's chunks of 4096 elements): two calls on the same
 * data give the same bits.  The work split depends on n, S and the offsets only.
 * workspace: ebfi_segment_stats_workspace(n, S) bytes (host arithmetic), 16-byte aligned, overwritten by every call.  Three
 * launches (the clearing of hist, the chunks, the per-segment fold) go onto `stream`, with no allocation and no host
 * synchronisation: capturable.
 * Null pointers, n < 0, S < 0, nb outside 1..2048, a misaligned workspace -> EBFI_ERR_ARG; a missing or short workspace ->
 * EBFI_ERR_WORKSPACE; a grid beyond 2^31 - 1 -> EBFI_ERR_UNSUPPORTED; none of them touches the GPU.  S == 0 is a no-op. */
int64_t ebfi_segment_stats_workspace(int64_t n, int S);
int ebfi_segment_stats(const float *x, int64_t n, const int64_t *offsets, int S, const double *limits, int nb, double *moments,
                       int32_t *hist, void *workspace, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ event simulator of the synthetic-dataset step
 * What generate_dataset/syn_gopro.py:77-81,115-116 asks of esim_py.EventSimulator: events from a run of gray uint8 frames.  esim_py
 * is not part of the reference tree; the law is stated here and restated in float64 numpy by tests/esim_ref.py, and the kernels
 * are bit-identical to that restatement.
 *
 * levels: 256 float64 on the HOST, the level L[v] of byte v (log(log_eps + v / 255.0) or v / 255.0), made by the caller: the
 * kernels never call log.  State per pixel, three float64 planes state[3][H][W] on the device: `it` (level of the last frame),
 * `ref` (last crossing level), `last_t` (time of the last emitted event; 0.0 = none yet).  ebfi_esim_init sets it = ref =
 * L[first frame], last_t = 0.  For each later frame at time T, dt = T - T_prev, itdt = L[v], all in float64:
 *   if |it - itdt| > 1e-6:
 *       pol = itdt >= it ? +1 : -1;  C = pol > 0 ? Cp : Cn;  cross = ref
 *       repeat: cross = cross + pol * C
 *               stop unless (pol > 0 and it < cross <= itdt) or (pol < 0 and it > cross >= itdt)
 *               t = T_prev + ((cross - it) * dt) / (itdt - it)          multiply, divide, add: three roundings, never fused
 *               if last_t == 0.0 or t - last_t >= refractory_period: emit (x, y, t, pol), last_t = t
 *               ref = cross
 *   it = itdt
 * The repeat is a counted loop of ebfi_esim_loop_bound(levels, Cp, Cn) = ceil((max L - min L) / min(Cp, Cn)) + 1 rounds (every
 * kept `cross` lies inside [min L, max L]), so no input can make a kernel spin.
 *
 * Frames: n later frames, uint8; pixel (k, y, x) at frames + k * frame_strides[0] + y * frame_strides[1] + x, or, with from_bgr,
 * its three bytes B, G, R at ... + 3 * x and gray = (4899 R + 9617 G + 1868 B + 8192) >> 14.  times: n + 1 float64 on the HOST,
 * times[0] the time of the frame the state stands at, times[k + 1] that of frame k, strictly increasing.  n <= EBFI_ESIM_MAX_CHUNK:
 * levels and times travel as kernel arguments, a longer sequence is fed in chunks with the state carried.
 *   ebfi_esim_count  walks the chunk from `state` WITHOUT writing it and stores counts[k][y][x] (int32), the number of events
 *                    pixel (y, x) emits in interval k.
 *   ebfi_esim_emit   takes the EXCLUSIVE prefix sums of counts (int64 offsets[k][y][x]), runs the identical walk, stores event e
 *                    of (k, y, x) at index offsets[k][y][x] + e of xs / ys (int16), ts (float64), ps (int8, +-1), and writes
 *                    the state back.  An index outside [0, capacity) is not stored (offsets that do not belong to the counts
 *                    cannot write out of bounds).  The layout is [k][y][x][emission], exact and deterministic: no atomics.
 * Output order of the law: (t, y, x, emission order within the pixel).  The emit layout is not yet that order, and a stable sort
 * on t alone is not always enough: an event of interval k + 1 can round onto T_k+1, where another pixel may have an interval-k
 * event exactly (linear levels and round thresholds produce both).  The caller sorts stably by pixel (y * W + x), then stably by t
 * (ebfi_amd.esim does, over all chunks of a call).
 * One lane owns one pixel, lanes run along x.  Each entry point is one launch on `stream`, no workspace, no host synchronisation;
 * n == 0 is a no-op.
 * Null pointers, n < 0 or > EBFI_ESIM_MAX_CHUNK, H or W outside [1, 32767], a negative stride, Cp or Cn below 1e-3, a non-finite
 * parameter or level (log_eps <= 0), a negative refractory period, times not strictly increasing, a loop bound beyond 2^24 ->
 * EBFI_ERR_ARG before anything touches the GPU (ebfi_esim_loop_bound returns -1 for them). */
#define EBFI_ESIM_MAX_CHUNK 128
int64_t ebfi_esim_loop_bound(const double *levels, double Cp, double Cn);
int ebfi_esim_init(const uint8_t *frame, int64_t row_stride, int from_bgr, int H, int W, const double *levels, double *state,
                   void *stream);
int ebfi_esim_count(const uint8_t *frames, const int64_t frame_strides[2], int from_bgr, int64_t n, int H, int W,
                    const double *times, const double *levels, double Cp, double Cn, double refractory_period,
                    const double *state, int32_t *counts, void *stream);
int ebfi_esim_emit(const uint8_t *frames, const int64_t frame_strides[2], int from_bgr, int64_t n, int H, int W,
                   const double *times, const double *levels, double Cp, double Cn, double refractory_period, double *state,
                   const int64_t *offsets, int64_t capacity, int16_t *xs, int16_t *ys, double *ts, int8_t *ps, void *stream);

/* ------------------------------------------------------------------ frame upsampling (adaptive Super-SloMo)
 * What generate_dataset/upsampling/utils/upsampler.py and model.py compute between the convolutions of their two U-Nets, at
 * batch 1 on planar float32 tensors [C, H, W] (csrc/upsample.hip; restated in float64 by tests/upsample_ref.py).  All run on
 * `stream`; none allocates or synchronises.
 *
 *   ebfi_avgpool2_forward      out[c][y][x] = mean of the 2 x 2 block of x [C, H, W] (H, W even)  -> [C, H/2, W/2]
 *   ebfi_bilinear_up2_forward  bilinear x2 with align_corners = True: source coordinate o * (n - 1) / (2n - 1), computed in
 *                              float32; a 1 x 1 map is copied to 2 x 2                             -> [C, 2H, 2W]
 *   ebfi_flow_max_magnitude    flow [4, H, W] = (F_0_1, F_1_0): *out = max over both of sqrt(u*u + v*v) in float32 (sum and sqrt
 *                              rounded separately).  A selection: the result is one of the magnitudes, whatever the order of
 *                              the reduction.  A NaN anywhere gives NaN.  The caller's N is ceil(*out).
 *
 * Back-warp of `img` by a flow (u, v), the reference's backWarp: at pixel (gx, gy) the coordinate x = 2 * ((gx + u) / W - 0.5),
 * likewise y with H, sampled by grid_sample(bilinear, zero padding, align_corners = True), i.e. at the pixel position
 * ((x + 1) / 2) * (W - 1) -- (gx + u) * (W - 1) / W up to rounding, so zero flow is NOT the identity.  Corners outside the image
 * contribute zero.
 *
 *   ebfi_slomo_assemble  with t in (0, 1) and, from Python doubles rounded to float32, c = -t(1-t):
 *                          F_t_0 = c F_0_1 + t^2 F_1_0,  F_t_1 = (1-t)^2 F_0_1 + c F_1_0
 *                        out20 [20, H, W] = I0 (3) | I1 (3) | F_0_1 (2) | F_1_0 (2) | F_t_1 (2) | F_t_0 (2) | warp(I1, F_t_1) (3)
 *                        | warp(I0, F_t_0) (3): the interpolation network's input.
 *   ebfi_slomo_blend     intrp [5, H, W] = that network's output, x20 = what assemble wrote:
 *                          F_t_0_f = intrp[0:2] + F_t_0, F_t_1_f = intrp[2:4] + F_t_1, V0 = sigmoid(intrp[4]), V1 = 1 - V0,
 *                          Ft_p = ((1-t) V0 warp(I0, F_t_0_f) + t V1 warp(I1, F_t_1_f)) / ((1-t) V0 + t V1)
 *                        rgb [3, H, W] (may be NULL) = Ft_p + mean; gray [H, W] = the byte law of that frame.
 *   ebfi_slomo_frame_u8  the byte law alone, of a normalised frame [3, H, W] (the reference writes I0 through it as well).
 *
 * Byte law, per channel c (RGB) in float32, each step rounded: m = v + mean[c] (mean = 0.429, 0.431, 0.397); s = 255 * m;
 * clip to [0, 255]; truncate to an integer level l[c] (a NaN gives 0).  gray = (3735 l[0] + 19235 l[1] + 9798 l[2] + 16384) >> 15:
 * OpenCV 4's 8-bit cvtColor(BGR2GRAY) as read from its source, NOT checked against a cv2 build; the reference passes its RGB
 * frame under the BGR code, so R takes the blue coefficient.
 *
 * assemble and blend need W % 4 == 0, H, W >= 2 and 16-byte aligned float tensors (gray: 4-byte); the others take any size.
 * Null pointers, non-positive or odd (pool) sizes, 2^31 elements or more, t outside (0, 1) -> EBFI_ERR_ARG. */
int ebfi_avgpool2_forward(const float *x, float *out, int C, int H, int W, void *stream);
int ebfi_bilinear_up2_forward(const float *x, float *out, int C, int H, int W, void *stream);
int ebfi_flow_max_magnitude(const float *flow, int H, int W, float *out, void *stream);
int ebfi_slomo_assemble(const float *I0, const float *I1, const float *flow, double t, float *out20, int H, int W, void *stream);
int ebfi_slomo_blend(const float *intrp, const float *x20, double t, float *rgb, uint8_t *gray, int H, int W, void *stream);
int ebfi_slomo_frame_u8(const float *frame, uint8_t *gray, int H, int W, void *stream);

/* ------------------------------------------------------------------ STGAN adversarial loss
 * 'GAN': Adversarial(PatchSize, gan_type='STGAN') of the reference's loss dictionary (train_ours.py:757-767,
 * loss/adversarial.py:68-168 over loss/discriminator.py:5-16, 208-263): a spatio-temporal patch discriminator D trained beside
 * the model by its own Adamax.  What is declared here is everything between D's convolutions (csrc/stgan.hip); the sixteen
 * convolutions are ebfi_conv2d_forward / _backward_data / _backward_weight* with EBFI_F32, called directly (ebfi_amd.gan).  tests/stgan_ref.py restates the law below in float64.
 *
 * The law.  block(ci, co, s) is, in order,
 *   Conv2d(ci, co, 3, stride = s, padding = 1, bias = False)
 *   BatchNorm2d(co): eps 1e-5, momentum 0.1, affine, ALWAYS batch statistics: per channel, mean and biased variance over the
 *     n = B H W values; running_mean <- 0.9 rm + 0.1 mean; running_var <- 0.9 rv + 0.1 var n / (n - 1);
 *     num_batches_tracked += 1
 *   LeakyReLU(0.2).
 * A branch with c input channels is block(c,8,1), (8,8,2), (8,16,1), (16,16,2), (16,32,1), (32,32,2), (32,64,1), (64,64,2).
 * s_features is a branch with c = 3 on f1; t_features a branch with c = 6 on cat([f1 - f0, f1 - f2], 1).  With q = P / 16 the
 * classifier flattens the s features to [B, 64 q^2], the t features likewise, concatenates them (s first) and applies
 * Linear(128 q^2, 1024), LeakyReLU(0.2), Linear(1024, 1): D(f0, f1, f2) is [B, 1].  P % 16 == 0 and H == W == P are required
 * (ValueError in Python, no device work); a stage with n == 1 (P = 16 at B = 1) is refused, as torch refuses it.
 * Adversarial(PatchSize, gan_type).forward(fake, real, input_frames) with f0, f2 = input_frames[:, 0], input_frames[:, 1]:
 *   1. d_fake = D(f0, fake.detach(), f2), then d_real = D(f0, real, f2): two passes, each with its own batch statistics; the
 *      running statistics are updated in that order.
 *   2. loss_d = mean(softplus(d_fake)) + mean(softplus(-d_real)), softplus in the stable form of BCE with logits:
 *      max(x, 0) - x y + log1p(exp(-|x|)) with target y.
 *   3. the gradients of D's parameters from zero, then ONE Adamax step as torch.optim.Adamax (lr 1e-3, betas (0.9, 0.999),
 *      eps 1e-8, weight_decay 0): exp_avg <- exp_avg + (1 - b1)(g - exp_avg); exp_inf <- max(b2 exp_inf, |g| + eps);
 *      p <- p - lr / (1 - b1^t) exp_avg / exp_inf.
 *   4. d_g = D(f0, fake, f2) with the UPDATED weights (a third running-statistics update); loss_g = mean(softplus(-d_g)) is
 *      returned with a graph into `fake` only.  (The reference also computes this pass's parameter gradients and zeroes them
 *      at the next call; they are not computed here.)
 *   5. self.loss is loss_d (gan_k = 1), kept as a device scalar.
 * Every other gan_type is refused (NotImplementedError) before any device work.
 *
 * Launch contract of every entry point of this section, as of ebfi_lpips_*_train: on `stream` only; no allocation, no host
 * synchronisation, no floating-point atomics -- the work split of every reduction depends on the shapes only, so two calls on
 * the same data give the same bits -- and an argument error touches no GPU.  Contiguous float32 tensors.
 *
 * ebfi_bn_lrelu_forward: x [B, C, HW] -> y = LeakyReLU_slope(gamma (x - mean) rstd + beta), per-channel mean and biased
 *   variance of the batch by a two-stage reduction in float64 (chunks of EBFI_BN_CHUNK values of a channel, one float64 pair
 *   each in the workspace, folded in a fixed order); stats float64 [C, 2] = (mean, rstd = 1 / sqrt(var + eps)) is what the
 *   backward reads; x - mean is taken in float64, so a plane with mean 100 and spread 0.1 keeps its variance and its
 *   normalised values.  running_mean / running_var float32 [C] (both or neither; NULL: not kept) and num_batches_tracked (one
 *   int64, may be NULL) are updated by the same call as written above.
 * ebfi_bn_lrelu_backward: with dy' = grad_y * (y > 0 ? 1 : slope) and xhat = (x - mean) rstd, the two per-channel sums
 *   s1 = sum dy', s2 = sum dy' xhat by the same reduction, then grad_x = gamma rstd (dy' - s1 / n - xhat s2 / n),
 *   grad_gamma = s2, grad_beta = s1 (float32 [C]; either may be NULL -- the generator's pass skips both).  x is the
 *   convolution's output, y what the forward wrote.
 * Both: 16-byte accesses when HW % 4 == 0 and the tensors are 16-byte aligned, scalar ones otherwise.  workspace:
 *   ebfi_bn_lrelu_workspace(B, C, HW) bytes (host arithmetic), 8-byte aligned, overwritten by every call.  Null pointers,
 *   sizes < 1, B HW == 1 -> EBFI_ERR_ARG; a missing / short workspace -> EBFI_ERR_WORKSPACE; C > 65535 or a grid beyond
 *   2^31 - 1 -> EBFI_ERR_UNSUPPORTED.
 * ebfi_stgan_temporal_forward: out [B, 2, CHW] = (f1 - f0, f1 - f2), each input with its own per-sample stride in elements
 *   (input_frames[:, k] is a strided view); ebfi_stgan_temporal_backward: the adjoint into f1 only,
 *   grad_f1 [B, CHW] = grad_t[:, 0] + grad_t[:, 1] (+ grad_s, the s branch's gradient, when not NULL), added left to right.
 * ebfi_linear_forward: y [B, N] = act(x [B, K] weight [N, K]^T + bias) (bias may be NULL; act 0 none, 1 LeakyReLU(slope)), one
 *   workgroup per output column and eight batch rows: float32 fma sums, a lane its quads of k in order, then a fixed tree.
 *   ebfi_linear_backward_data: grad_x [B, K] = grad_y [B, N] weight, times LeakyReLU'(mask_y) when mask_y [B, K] (the layer
 *   below's output) is not NULL; ebfi_linear_backward_weight: grad_weight [N, K] = grad_y^T x and grad_bias [N] (may be NULL),
 *   summed over the batch in order.  The classifier's two layers are skinny products (B rows against up to 1024 x 32768
 *   weights, read once per eight rows); they are native so that every sum has one owner and a fixed order -- a captured step
 *   replays the bits of an eager one, which the BLAS behind torch.nn.functional.linear did not do here.
 *   B <= 524280, N <= 65535, K < 2^31, else EBFI_ERR_UNSUPPORTED.
 * ebfi_bce_logits_pair: loss[0] = mean softplus(fake) + mean softplus(-real) over n logits each (float64 sums, one
 *   workgroup, fixed order); a NULL side contributes nothing (loss_g = the call with fake NULL and real = d_g);
 *   grad_fake = sigmoid(fake) / n, grad_real = (sigmoid(real) - 1) / n (either may be NULL).
 * ebfi_adamax_step: the update of step 3 over one flat buffer of n elements, in place, in torch's float32 operations;
 *   weight_decay != 0: g' = g + weight_decay p first.  grad2 (may be NULL): a second gradient buffer added to the first in
 *   registers (the fake and the real pass leave one each), neither is written.  step: a device float holding the ALREADY
 *   incremented count; the bias correction is taken in double.  Hyper-parameters travel by value.  All buffers 16-byte
 *   aligned; the n % 4 last elements by scalar accesses. */
#define EBFI_BN_CHUNK 4096
int64_t ebfi_bn_lrelu_workspace(int64_t B, int C, int64_t HW);
int ebfi_bn_lrelu_forward(const float *x, const float *gamma, const float *beta, float *y, double *stats, float *running_mean,
                          float *running_var, int64_t *num_batches_tracked, int64_t B, int C, int64_t HW, double eps,
                          double momentum, double slope, void *workspace, int64_t workspace_bytes, void *stream);
int ebfi_bn_lrelu_backward(const float *grad_y, const float *x, const float *y, const float *gamma, const double *stats,
                           float *grad_x, float *grad_gamma, float *grad_beta, int64_t B, int C, int64_t HW, double slope,
                           void *workspace, int64_t workspace_bytes, void *stream);
int ebfi_stgan_temporal_forward(const float *f0, int64_t f0_stride, const float *f1, int64_t f1_stride, const float *f2,
                                int64_t f2_stride, float *out, int64_t B, int64_t CHW, void *stream);
int ebfi_stgan_temporal_backward(const float *grad_t, const float *grad_s, float *grad_f1, int64_t B, int64_t CHW, void *stream);
int ebfi_linear_forward(const float *x, const float *weight, const float *bias, float *y, int64_t B, int64_t K, int64_t N, int act,
                        double slope, void *stream);
int ebfi_linear_backward_data(const float *grad_y, const float *weight, const float *mask_y, double slope, float *grad_x, int64_t B,
                              int64_t K, int64_t N, void *stream);
int ebfi_linear_backward_weight(const float *grad_y, const float *x, float *grad_weight, float *grad_bias, int64_t B, int64_t K,
                                int64_t N, void *stream);
int ebfi_bce_logits_pair(const float *fake, const float *real, int64_t n, float *loss, float *grad_fake, float *grad_real,
                         void *stream);
int ebfi_adamax_step(float *param, const float *grad, const float *grad2, float *exp_avg, float *exp_inf, const float *step,
                     int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, void *stream);

/* ------------------------------------------------------------------ the rest of dataloader/encodings.py: ordered scatters
 * ebfi_events_to_grid: an event list (xs, ys, ts, ps: float32 [n] on the device; ts sorted ascending where a mode reads it) ->
 * out float32 [planes, oH, oW], every element written.  The reference builds all of these with index_put_(accumulate=True) of
 * fractional weights; THE LAW is what that call computes with one thread (or under torch.use_deterministic_algorithms): every
 * pixel receives its addends in EVENT-LIST ORDER, each product and sum rounded to fp32, nothing fused, denormals kept.  The
 * library reaches it without a float atomic: a stable radix sort of (pixel key, event index) with integer histograms, integer
 * scans and ballot ranks (csrc/encodings.hip), then one thread per (pixel, plane) that walks its pixel's run in ascending event
 * index.  Two calls on the same input give the same bits; a pixel that owns every event costs the sort nothing extra and the
 * accumulation one serial walk per plane.  The index is built once per call and serves all planes.
 * Out-of-range events (x < 0, x >= W, y < 0, y >= H; a NaN coordinate counts as out of range) follow what the reference's
 * IN-PLACE zeroing (xs = ys = 0 and the weight it was handed = 0) does to its own later passes.  The caller's arrays are never
 * written; the effect on the output is reproduced per mode (`bins` = planes unless stated):
 *   EBFI_GRID_IMAGE             events_to_image / events_to_image_torch(interpolation=None); bins = 1.  out[y][x] += p, truncated
 *                               coordinates; an out-of-range event adds 0 at (0,0).
 *   EBFI_GRID_VOXEL_BILINEAR    events_to_voxel_torch(temporal_bilinear=True): dt = ts[n-1] - ts[0] + 1e-6f,
 *                               t = (ts - ts[0]) / dt * (bins - 1), plane b adds p * max(0, 1 - |t - b|).  The weights are a
 *                               fresh tensor per bin but xs / ys are the caller's: rule 1 -- an out-of-range event adds nothing
 *                               in bin 0 and its FULL weight at pixel (0,0) in every later bin.  n <= 3 or all stamps zero
 *                               (sorted non-negative stamps: ts[0] == ts[n-1] == 0, decided on the device) -> zeros.
 *   EBFI_GRID_VOXEL_NORMALISED  events_to_voxel: stamps already in [0, 1], t = ts * (bins - 1); rule 1 again; no n <= 3 exit.
 *   EBFI_GRID_VOXEL_NAIVE       events_to_voxel_torch(temporal_bilinear=False) and
 *   EBFI_GRID_STACK_NO_POLARITY events_to_stack_no_polarity (one law): plane b adds p for the events of the slice [beg, end)
 *                               that the reference's fp32 bin edges and its own binary search give (end = r + 1: neighbouring
 *                               bins share edge events).  ps[beg:end] is a view: rule 2 -- the first bin that holds an
 *                               out-of-range event zeroes its polarity for good, so it adds 0 in every bin.  Same zero exits.
 *   EBFI_GRID_CHANNELS          events_to_channels; bins = 2.  Plane 0 adds p * (p < 0 ? 0 : p), plane 1 adds p * (p > 0 ? 0 : p).
 *                               The products are temporaries, the coordinates are not: rule 3 -- the positive pass drops an
 *                               out-of-range event and moves it, the negative pass counts it at (0,0) (events_to_stack's quirk).
 *   EBFI_GRID_MASK              events_to_mask; bins = 1.  index_put_(accumulate=False) with duplicates: rule 4 -- the LAST
 *                               event of a pixel wins, |p|; an out-of-range last writer stores 0 at (0,0).
 *   EBFI_GRID_BILINEAR_PADDED   events_to_image_torch(interpolation='bilinear', padding=True): out [H+1, W+1]; bins = 1
 *   EBFI_GRID_BILINEAR_CLIPPED  (..., padding=False, clip_out_of_range=True): out [H, W]; events with x >= W - 1 or y >= H - 1
 *                               are masked to weight 0 at (0,0).  Both: px = floor(x), dx = x - px, four index_put_ in turn, so a
 *                               pixel's sum is every top-left addend (w * (1 - dx)) * (1 - dy) in event order, then the
 *                               top-right (w * dx) * (1 - dy), bottom-left (w * (1 - dx)) * dy and bottom-right (w * dx) * dy ones.
 *                               (padding=False without clipping raises IndexError in the reference: there is no mode for it.)
 * ebfi_interpolate_to_image: the same four-pass law IN PLACE on img float32 [H, W] (its old value first), base pixels
 * pxs / pys int64, fractions and weights float32.  An event whose 2 x 2 footprint leaves the image is skipped (the reference
 * raises IndexError or, for negative indices, wraps).
 * workspace: ebfi_events_grid_workspace(n, bins, H, W) bytes for both (host arithmetic; 0 for bad or unsupported sizes; with
 * bins = 1 and the image's H, W for ebfi_interpolate_to_image), 16-byte aligned, overwritten by every call.  Per call: the key
 * kernel, four launches per 8 key bits, the run starts, (the bin edges,) the accumulation -- all on `stream`, one chain, no
 * allocation, nothing read back: capturable.
 * Null pointers, n < 0, bins / H / W < 1, an unknown mode, bins that contradict the mode, a misaligned workspace -> EBFI_ERR_ARG;
 * a missing or short workspace -> EBFI_ERR_WORKSPACE; n > 2^31 - 257, (H+1) * (W+1) > 2^31 - 2 or bins > 65535 ->
 * EBFI_ERR_UNSUPPORTED; none of them touches the GPU.  n == 0 gives zeros (ebfi_interpolate_to_image: a no-op). */
enum {
    EBFI_GRID_IMAGE = 0,
    EBFI_GRID_VOXEL_BILINEAR = 1,
    EBFI_GRID_VOXEL_NORMALISED = 2,
    EBFI_GRID_VOXEL_NAIVE = 3,
    EBFI_GRID_STACK_NO_POLARITY = 4,
    EBFI_GRID_CHANNELS = 5,
    EBFI_GRID_MASK = 6,
    EBFI_GRID_BILINEAR_PADDED = 7,
    EBFI_GRID_BILINEAR_CLIPPED = 8
};
int64_t ebfi_events_grid_workspace(int64_t n, int bins, int H, int W);
int ebfi_events_to_grid(const float *xs, const float *ys, const float *ts, const float *ps, int64_t n, int mode, int bins, int H,
                        int W, float *out, void *workspace, int64_t workspace_bytes, void *stream);
int ebfi_interpolate_to_image(const int64_t *pxs, const int64_t *pys, const float *dxs, const float *dys, const float *weights,
                              int64_t n, int H, int W, float *img, void *workspace, int64_t workspace_bytes, void *stream);
/* get_hot_event_mask's loop in one launch (one workgroup): mask float32 [H, W] := 1, then up to max_px times "the first flat
 * index of the maximum of event_rate (a NaN is the maximum, as in torch.argmax); if its value > max_rate, clear it in event_rate
 * AND in mask, else stop".  event_rate float32 [H, W] is edited in place -- that is the function's purpose.  max_px == 0 only
 * fills the mask.  Null pointers, H / W < 1, max_px < 0 -> EBFI_ERR_ARG. */
int ebfi_hot_event_mask(float *event_rate, int H, int W, int max_px, float max_rate, float *mask, void *stream);
/* stack2cnt: stack float32 [B, TB, plane] -> cnt float32 [B, 2, plane]: r = rintf(value) (half to even); cnt[b][0] sums
 * (r < 0 ? 0 : r) and cnt[b][1] sums -(r > 0 ? 0 : r) over the bin axis in bin order, fp32. */
int ebfi_stack_to_cnt(const float *stack, int64_t B, int TB, int64_t plane, float *cnt, void *stream);
/* events_polarity_mask: out float32 [2, n], row 0 = (p < 0 ? 0 : p), row 1 = -(p > 0 ? 0 : p) (the caller transposes). */
int ebfi_polarity_mask(const float *ps, int64_t n, float *out, void *stream);

/* ------------------------------------------------------------------ loss/flow.py and myutils/iwe.py: images of warped events
 * events float32 [B, N, 4] = (ts, y, x, p) per event (the code's layout; the reference's docstrings say otherwise); flow maps
 * float32 [B, 2, H, W] given by their four strides in ELEMENTS (channel 1 is the vertical component); masks float32, one value
 * per event, `mask_stride` elements apart (pol_mask [B, N, 2]: the pointer, the pointer + 1, stride 2).  csrc/iwe.hip.
 * THE LAW.  The reference builds every image with scatter_add_ along dim 1; with one thread that is a serial walk, so each
 * pixel receives its addends in ASCENDING LIST POSITION, every product and sum rounded to fp32, nothing fused.  As for
 * ebfi_events_to_grid: key = b * H * W + idx per list entry, a stable radix sort of (key, position), one thread per pixel
 * adding its run in order, each plane its own chain (a run of 64 or more: gathered by the wave, summed in lane order).  No
 * float atomics.
 * ebfi_iwe_get_interpolation: flow_ev [B, N, 2] = (y, x) flow per event -> idx, weights float32 [B, M] (M = N with round_idx,
 *   else 4 N: top-left, top-right, bottom-left, bottom-right lists one after the other).  warped = pos + (((tref - ts) * flow)
 *   * flow_scaling); corners floor(w), floor(w + 1); weight max(0, 1 - |w - corner|) per axis, y times x; round_idx: rintf (half
 *   to even), weight 1.  A corner with y < 0, y >= H, x < 0 or x >= W gets index 0 and weight 0 (the reference: -0.0 where the
 *   coordinate was negative); so does a non-finite warped coordinate (the reference's .long() of it is undefined).
 * ebfi_iwe_interpolate: idx [B, M] float32 or int64 (idx_is_i64), weights [B, M], polarity_mask [B, M] or NULL -> out
 *   [B, 1, H, W] = the ordered scatter of weights * polarity_mask (its own rounding).  An index outside [0, H * W) is DROPPED
 *   (the reference raises).  Workspace: ebfi_iwe_workspace(B, ceil(M / 4), H, W).
 * ebfi_iwe_deblur: deblur_events (planes = 1, out [B, 1, H, W]; mask_a may be NULL, mask_b is not read) and compute_pol_iwe
 *   (planes = 2, both masks, out [B, 2, H, W]) in one call: the flow is gathered at each event's source pixel y * W + x, the events are warped to tref = 1
 *   and scattered with one sort for both masks.  An event whose source pixel is outside the image or not integral takes flow 0
 *   and weight 0 (the reference's gather raises or asserts).
 * ebfi_iwe_warping_forward: the loss of EventWarping for ONE flow -> *loss (float32 device scalar) and images float32
 *   [2 (tref = 1, tref = 0)][B][4 (count+, count-, stamp-weighted sum+, sum-)][H * W], kept by the caller for the backward
 *   call.  One sort per direction serves its four images; stamp weight (w * ts) * mask forward, (w * (1 - ts)) * mask
 *   backward; loss = sum of (sum / (count + 1e-9f))^2 over both directions and polarities + weight * (sum of
 *   sqrt(d^2 + 1e-6) over the differences of the flow along both axes), the squares, roots and both reduction stages in
 *   float64, in a fixed order.  A NaN in the flow reaches the loss through the smoothness term.
 * ebfi_iwe_source_index: the events sorted by SOURCE pixel into `index` (ebfi_iwe_index_bytes(B, N, H, W) bytes -- B N entries,
 *   far smaller than the workspace --, 16-byte aligned, caller-owned, read by every backward call on these events: it does
 *   not depend on the flow).
 * ebfi_iwe_warping_backward: grad_flow float32 [B, 2, H, W] (contiguous, every element written once) = *grad_out * d loss /
 *   d flow.  No scatter: one thread per source pixel walks its events in list order, recomputes the corners of both
 *   directions, reads 2 r (t - r) / (C + 1e-9f) with r = A / (C + 1e-9f) at each corner and polarity, applies the weight's
 *   derivative (torch's subgradients: abs'(0) = 0, a tie of max(0, a) passes half) and (tref - ts) * flow_scaling, adds
 *   forward then backward, then the smoothness gradient from up to four neighbours; float64 accumulation.
 * ebfi_iwe_averaged: AveragedIWE -> out [B, 2, H, W]: rounded warp to tref = 1, per-polarity counts by the ordered scatter,
 *   each divided, where positive, by the number of distinct source pixels among the feasible events of that pixel and
 *   polarity (p < 1 is negative; weight 0 means ignored; pol_mask does not enter that number, as in the reference).
 * Workspace: ebfi_iwe_workspace(B, N, H, W) bytes (host arithmetic; 0 for bad or unsupported sizes), 16-byte aligned,
 * overwritten by every call; all launches on `stream`, one chain, nothing allocated or read back: capturable.
 * Null pointers, B < 1, N < 0, H / W < 1, a misaligned workspace -> EBFI_ERR_ARG; a missing or short workspace ->
 * EBFI_ERR_WORKSPACE; 4 * B * N >= 2^32 or B * H * W >= 2^32 - 1 -> EBFI_ERR_UNSUPPORTED; none touches the GPU. */
int64_t ebfi_iwe_workspace(int64_t B, int64_t N, int H, int W);
int64_t ebfi_iwe_index_bytes(int64_t B, int64_t N, int H, int W);
int ebfi_iwe_get_interpolation(const float *events, const float *flow_ev, int64_t B, int64_t N, float tref, int H, int W,
                               float flow_scaling, int round_idx, float *idx, float *weights, void *stream);
int ebfi_iwe_interpolate(const void *idx, int idx_is_i64, const float *weights, const float *polarity_mask, int64_t B, int64_t M,
                         int H, int W, float *out, void *workspace, int64_t workspace_bytes, void *stream);
int ebfi_iwe_deblur(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw, const float *events,
                    int64_t B, int64_t N, int H, int W, float flow_scaling, int round_idx, int planes, const float *mask_a,
                    const float *mask_b, int64_t mask_stride, float *out, void *workspace, int64_t workspace_bytes, void *stream);
int ebfi_iwe_source_index(const float *events, int64_t B, int64_t N, int H, int W, void *index, int64_t index_bytes, void *stream);
int ebfi_iwe_warping_forward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                             const float *events, const float *pol_mask, int64_t B, int64_t N, int H, int W, float flow_scaling,
                             double weight, float *images, float *loss, void *workspace, int64_t workspace_bytes, void *stream);
int ebfi_iwe_warping_backward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                              const float *events, const float *pol_mask, int64_t B, int64_t N, int H, int W, float flow_scaling,
                              double weight, const float *images, const void *index, int64_t index_bytes, const float *grad_out,
                              float *grad_flow, void *stream);
int ebfi_iwe_averaged(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw, const float *events,
                      const float *pol_mask, int64_t B, int64_t N, int H, int W, float flow_scaling, float *out, void *workspace,
                      int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ loss/reconstruction.py and myutils/gradients.py
 * BrightnessConstancy's three terms and the Sobel operator, with their gradients.  csrc/bcloss.hip.  Images are float32,
 * contiguous, one channel: [B, 1, H, W] (Sobel and the total variation: `planes` images [H, W]); flow maps float32 [B, 2, H, W]
 * given by their four strides in ELEMENTS (channel 0 horizontal, channel 1 vertical), in units of S = flow_scaling = max(H, W).
 * THE LAW.  Pixel (h, w) samples at ix = ((gx + 1) * W - 1) / 2 with gx = 2 * (w - fx * S) / (W - 1) - 1, and iy alike with H
 * (grid_sample without align_corners -- not w - fx * S), bilinear, corners outside the image contribute 0; a coordinate that is
 * not finite samples 0 and passes no gradient.  The per-pixel arithmetic is float64 of the float32 inputs; every loss is a
 * float64 sum in two stages of fixed order -> *loss, a float32 device scalar.  The gradient into the flow is a gather; the
 * gradient into the SAMPLED image is the scatter, as an ordered sum: every destination pixel adds its float32 addends in
 * ascending source-pixel index, then corner order top-left, top-right, bottom-left, bottom-right, fp32 and unfused -- a stable
 * radix sort of the 4 B H W (destination, source) entries and one thread per destination, as for ebfi_iwe_* (a run of 64 or
 * more: gathered by the wave, summed in lane order).  No float atomics.
 * ebfi_sobel_forward: x [planes, H, W] -> gradx, grady [planes, H, W]: replication pad of one pixel, correlation with
 *   [[-1,0,1],[-2,0,2],[-1,0,1]] and [[-1,-2,-1],[0,0,0],[1,2,1]], divided by 8.  ebfi_sobel_backward: the adjoint as a
 *   gather -> grad_x (every element written); either incoming gradient may be NULL, not both.
 * ebfi_bc_mask_flow: masked [B, 2, H, W] contiguous = flow * m with m = 1 where the channel sum s of cnt [B, C, H, W] (added in
 *   channel order, fp32) is positive and s itself elsewhere: the flow AveragedIWE reads.  It is the generative term's third
 *   launch beside the pixel kernel and the final reduction: csrc/iwe.hip is pinned by a host test and takes no mask.
 * ebfi_bc_generative_forward: with the masked flow f (recomputed per pixel), the Sobel values of the four corners from the
 *   4 x 4 window of img with clamped coordinates, pred = (Sx fx + Sy fy) * S, resid [B, H, W] = (avg[:, 0] - avg[:, 1]) + pred
 *   (avg [B, 2, H, W]: AveragedIWE of the masked flow), *loss = sum resid^2.  resid is kept by the caller for
 * ebfi_bc_generative_backward: grad_flow [B, 2, H, W] contiguous = m * d loss / d f (through the product and through the grid;
 *   exactly +0 where m == 0) and grad_img [B, 1, H, W] = the ordered scatter into the two Sobel gradient images, then the
 *   Sobel adjoint.  Either may be NULL (not both); without grad_img nothing is sorted and the forward workspace suffices.
 *   No gradient through avg.
 * ebfi_bc_temporal_forward: resid = img - sample(prev_img) under the flow as given, *loss = weight * sum |resid|.
 * ebfi_bc_temporal_backward: grad_flow, grad_prev (the ordered scatter) and grad_img = weight * *grad_out * sign(resid), sign(0)
 *   = 0; each may be NULL, not all; the full workspace is needed only with grad_prev.
 * ebfi_bc_tv_forward / _backward: *loss = weight * (sum |x[h] - x[h + 1]| + sum |x[w] - x[w + 1]|) per image; the gradient is a
 *   gather from up to four neighbours.
 * Workspace: ebfi_bc_workspace(B, H, W) bytes for a backward call, ebfi_bc_forward_workspace(B, H, W) (its first part: the
 * partial sums) for a forward call -- host arithmetic, 0 for bad or unsupported sizes --, 16-byte aligned, overwritten by every
 * call; all launches on `stream`, one chain, nothing allocated or read back: capturable.
 * Null pointers, B < 1, C < 1, H < 2 or W < 2 (the law divides by n - 1), a misaligned workspace -> EBFI_ERR_ARG; a missing or
 * short workspace -> EBFI_ERR_WORKSPACE; 4 * B * H * W >= 2^32 for the entry points of the two sampling terms and
 * ebfi_bc_mask_flow (entry positions of the sort are 32-bit), planes * H * W >= 2^32 - 1 for Sobel and the total variation, which
 * sort nothing -> EBFI_ERR_UNSUPPORTED; none touches the GPU. */
int64_t ebfi_bc_workspace(int64_t B, int H, int W);
int64_t ebfi_bc_forward_workspace(int64_t B, int H, int W);
int ebfi_sobel_forward(const float *x, int64_t planes, int H, int W, float *gradx, float *grady, void *stream);
int ebfi_sobel_backward(const float *grad_gradx, const float *grad_grady, int64_t planes, int H, int W, float *grad_x, void *stream);
int ebfi_bc_mask_flow(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw, const float *cnt, int C,
                      int64_t B, int H, int W, float *masked, void *stream);
int ebfi_bc_generative_forward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                               const float *img, const float *cnt, int C, const float *avg, int64_t B, int H, int W,
                               float flow_scaling, float *resid, float *loss, void *workspace, int64_t workspace_bytes, void *stream);
int ebfi_bc_generative_backward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                                const float *img, const float *cnt, int C, const float *resid, int64_t B, int H, int W,
                                float flow_scaling, const float *grad_out, float *grad_flow, float *grad_img, void *workspace,
                                int64_t workspace_bytes, void *stream);
int ebfi_bc_temporal_forward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                             const float *prev_img, const float *img, int64_t B, int H, int W, float flow_scaling, double weight,
                             float *resid, float *loss, void *workspace, int64_t workspace_bytes, void *stream);
int ebfi_bc_temporal_backward(const float *flow, int64_t flow_sb, int64_t flow_sc, int64_t flow_sh, int64_t flow_sw,
                              const float *prev_img, const float *resid, int64_t B, int H, int W, float flow_scaling, double weight,
                              const float *grad_out, float *grad_flow, float *grad_prev, float *grad_img, void *workspace,
                              int64_t workspace_bytes, void *stream);
int ebfi_bc_tv_forward(const float *img, int64_t planes, int H, int W, double weight, float *loss, void *workspace,
                       int64_t workspace_bytes, void *stream);
int ebfi_bc_tv_backward(const float *img, int64_t planes, int H, int W, double weight, const float *grad_out, float *grad_img,
                        void *stream);

/* ------------------------------------------------------------------ models/model_misc/unet.py: what lies between the convolutions
 * The ConvLSTM and ConvGRU cell tails of models/model_misc/submodules.py and UpsampleConvLayer's bilinear up-sampling, each with
 * its gradient.  csrc/recurrent.hip.  Tensors are float32, contiguous [B, channels, H, W]; HW = H * W.  One launch per call on
 * `stream`, nothing allocated or read back, NO atomics: capturable and bit-reproducible.  16-byte accesses when HW % 4 == 0 and
 * every tensor is 16-byte aligned, scalar ones otherwise.  float32, no contraction; with e = expf(-|v|), sigmoid(v) and
 * 1 - sigmoid(v) are 1 / (1 + e) and e / (1 + e) (swapped for v < 0), and 1 - tanh(v)^2 past |v| = 0.625 is 4 e' / (1 + e')^2,
 * e' = expf(-2 |v|): no complement is formed by subtracting from 1, so a saturated gate keeps its derivative's accuracy.
 * ebfi_lstm_cell_forward: gates [B, 4C, HW] are the pre-activations in chunk order in, remember, out, cell; with i, f, o their
 *   sigmoids and g = tanh(cell gate): cell = f * prev_cell + i * g, hidden = o * tanh(cell).  prev_cell NULL = zeros.
 * ebfi_lstm_cell_backward: from gates, prev_cell (NULL = zeros), the saved cell and grad_hidden / grad_cell (either NULL = zero)
 *   -> grad_gates [B, 4C, HW], the gradient of the PRE-activations, and grad_prev_cell (NULL = not wanted).  The sigmoids and
 *   both tanh are recomputed: d = grad_cell + grad_hidden o (1 - tanh(cell)^2); (d g i (1 - i), d prev_cell f (1 - f),
 *   grad_hidden tanh(cell) o (1 - o), d i (1 - g^2)); grad_prev_cell = d f.
 * ebfi_gru_reset_forward: out [B, Cx + C, HW] = cat(x [B, Cx, HW], h * sigmoid(reset_pre)) -- the input of the out-gate
 *   convolution, written once.  h NULL = zeros (reset_pre is then not read).
 * ebfi_gru_reset_backward: grad_out [B, Cx + C, HW] -> grad_x = its first Cx channels (NULL = not wanted), grad_reset_pre =
 *   g h r (1 - r) and grad_h = grad_h_in + g r (g the last C channels, r = sigmoid(reset_pre); grad_h_in, the direct term of
 *   the second half, may be NULL = zero; grad_h NULL = not wanted).  h NULL: grad_reset_pre and grad_h are zeros.
 * ebfi_gru_update_forward: new_state = h * (1 - u) + tanh(out_pre) * u with u = sigmoid(update_pre); h NULL = zeros.
 * ebfi_gru_update_backward: grad_update_pre = g (t - h) u (1 - u), grad_out_pre = g u (1 - t^2), grad_h = g (1 - u) (NULL = not
 *   wanted), t = tanh(out_pre).
 * ebfi_bilinear_up_forward: x [planes, H, W] -> out [planes, scale H, scale W], scale 2 or 4, the law of F.interpolate(mode =
 *   'bilinear', align_corners = False): source coordinate (o + 0.5) / scale - 0.5, a negative one clamped to 0, i0 its integer
 *   part, i1 = i0 + 1 below n - 1 (else i0), weights 1 - fraction and fraction.
 * ebfi_bilinear_up_backward: the adjoint as a gather: every input pixel adds (wy * wx) * grad_out over its contributors
 *   o in [scale i - scale / 2, scale i + 3 scale / 2 - 1] per axis, rows ascending, then columns ascending, in float32.
 * A null required pointer, B / C / Cx / HW / planes / H / W < 1, a scale other than 2 or 4 -> EBFI_ERR_ARG; nothing is launched. */
int ebfi_lstm_cell_forward(const float *gates, const float *prev_cell, float *hidden, float *cell, int64_t B, int C, int64_t HW,
                           void *stream);
int ebfi_lstm_cell_backward(const float *gates, const float *prev_cell, const float *cell, const float *grad_hidden,
                            const float *grad_cell, float *grad_gates, float *grad_prev_cell, int64_t B, int C, int64_t HW, void *stream);
int ebfi_gru_reset_forward(const float *reset_pre, const float *x, const float *h, float *out, int64_t B, int Cx, int C, int64_t HW,
                           void *stream);
int ebfi_gru_reset_backward(const float *grad_out, const float *reset_pre, const float *h, const float *grad_h_in, float *grad_x,
                            float *grad_reset_pre, float *grad_h, int64_t B, int Cx, int C, int64_t HW, void *stream);
int ebfi_gru_update_forward(const float *update_pre, const float *out_pre, const float *h, float *new_state, int64_t B, int C, int64_t HW,
                            void *stream);
int ebfi_gru_update_backward(const float *update_pre, const float *out_pre, const float *h, const float *grad_new, float *grad_update_pre,
                             float *grad_out_pre, float *grad_h, int64_t B, int C, int64_t HW, void *stream);
int ebfi_bilinear_up_forward(const float *x, float *out, int64_t planes, int H, int W, int scale, void *stream);
int ebfi_bilinear_up_backward(const float *grad_out, float *grad_x, int64_t planes, int H, int W, int scale, void *stream);

/* ------------------------------------------------------------------ per-kernel device timing
 * When enabled, every launch made by this library is bracketed by a hipEvent pair recorded on the
 * launch stream.  ebfi_prof_collect() must be called after the stream(s) are synchronised; it
 * folds the pending pairs into per-kernel totals and frees their slots (totals keep accumulating until
 * ebfi_prof_reset), so a long run collects once per step.  Pending slots between two collects are bounded
 * (default EBFI_PROF_MAX_PENDING, ebfi_prof_set_capacity changes it); launches beyond the bound are not
 * timed and are counted in *dropped -- callers must treat dropped != 0 as a failed measurement.
 * Labels are "<kernel symbol>" or "<kernel symbol>/<role>" when one kernel serves several ops
 * (e.g. "conv_fwd_bf16x3_db/fwd" and "conv_fwd_bf16x3_db/dgrad"). */
#define EBFI_PROF_MAX_PENDING 65536
void ebfi_prof_enable(int on);
int ebfi_prof_set_capacity(int max_pending);
void ebfi_prof_reset(void);
int ebfi_prof_collect(int *dropped);
int ebfi_prof_num_kernels(void);
int ebfi_prof_get(int index, const char **name, int64_t *launches, double *total_ms);
/* algorithmic work (SURVEY.md 8(d) formulas) summed over the timed launches of kernel `index` */
int ebfi_prof_get_work(int index, double *flops, double *bytes);

#ifdef __cplusplus
}
#endif
#endif /* EBFI_HIP_H */
