/*
 * ideepcolor.h -- C ABI of libideepcolor_hip.so: the MI355X (gfx950) implementation of the
 * Local-Hints colorization forward pass.
 *
 * The reference has NO FFI/plugin interface for this path: the boundary is the
 * duck-typed Python class in data/colorize_image.py whose net_forward() calls
 *     self.net.forward(self.img_l_mc, self.input_ab_mc, self.input_mask_mult, self.mask_cent)
 * at data/colorize_image.py:263 (torch backend) / :427-428 (caffe backend).  Everything below
 * replaces exactly that call and the module it lands in, models/pytorch/model.py:134-175
 * (SIGGRAPHGenerator.forward).  Each entry point cites what it stands in for.
 *
 * Conventions: extern "C", plain pointers and sizes, no torch/C++ types.  Every function returns
 * IDC_OK (0) or a negative idc_status; idc_last_error() gives the text.  Host tensors are NCHW
 * fp32, C-contiguous, caller-owned (the layout of the reference's torch tensors).  A handle owns
 * one device, one stream, all device memory; it is not thread-safe; distinct handles are
 * independent.  There is no CPU fallback: without a gfx950 device idc_create fails.
 */
#ifndef IDEEPCOLOR_H
#define IDEEPCOLOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IDC_VERSION 2   /* (round 6 adds precisions 2 / 3 without a bump: older blobs stay valid) 2: blob header flags may carry IDC_FLAG_THROUGHPUT_BLOB; round-3 blobs (Winograd images added without a bump) were 1 */

typedef struct idc_context* idc_handle;

typedef enum idc_status {
    IDC_OK = 0,
    IDC_ERR_INVALID_ARG = -1,
    IDC_ERR_NO_DEVICE = -2,     /* no HIP device / not gfx950 */
    IDC_ERR_HIP = -3,           /* a HIP runtime call failed */
    IDC_ERR_NO_WEIGHTS = -4,    /* forward before weights (reference: "I need to have a net!", colorize_image.py:88-90) */
    IDC_ERR_MISSING_KEY = -5,   /* a state_dict key of SURVEY.md Appendix B is absent or mis-shaped */
    IDC_ERR_BATCH = -6,         /* n > max_batch or n <= 0 */
    IDC_ERR_UNSUPPORTED = -7,
    IDC_ERR_INTERNAL = -8       /* a kernel variant was selected for a launch it does not cover: a bug in the library, reported instead of
                                 * falling back to another kernel with the wrong weight image */
} idc_status;

/* Arithmetic type of the conv stack.  BF16: bf16 activations+weights, fp32 MFMA accumulation,
 * fp32 bias/BN/shortcut sums.  FP32: exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) end to end.      */
typedef enum idc_precision { IDC_FP32 = 0, IDC_BF16 = 1, IDC_BF16X3 = 2, IDC_BF16X6 = 3, IDC_FP16X3 = 4, IDC_FP16 = 5 } idc_precision;
/* BF16X3 / BF16X6 (round 6): the fp32 contract of colorize_image.py:263 carried on the bf16 matrix pipe.  Every fp32 operand travels as a sum of
 * bf16 values -- x = hi + lo (X3) or hi + mid + lo (X6: all 24 mantissa bits) -- and a product x*w is the sum of the bf16 products that matter:
 * hi.hi + lo.hi + hi.lo (three v_mfma_f32_16x16x32_bf16 per fragment pair, 2^-16 relative), or those + mid.hi + hi.mid + mid.mid (six, 2^-24:
 * fp32-equivalent), all into ONE fp32 accumulator set.  Activations between layers are stored split (2 or 3 bf16 planes per pixel), bias / BN /
 * shortcut sums / the tanh head stay fp32, model1 (4 -> 64 -> 64 channels, 3 % of the MACs) runs on the exact-fp32 kernels.  Throughput path:
 * every layer runs the large-tile kernels whatever the batch (the batch-1 click path keeps IDC_FP32 / IDC_BF16).  Error against the float64
 * oracle: X6 at or below IDC_FP32's, X3 <= 1e-3 on the +-110 ab map with torch-default-init weights (tests/bounds.py).
 * FP16X3 (round 6): BF16X3's planes, segments and kernels with FP16 parts -- x = hi + lo with 11-bit hi and lo (22 bits, 2^-22 relative per
 * operand instead of 2^-16), three v_mfma_f32_16x16x32_f16 per fragment pair.  A layer's weight parts hold w * 2^s, s the power of two that brings
 * the layer's largest weight into [8192, 16384) (exact; the accumulators are multiplied by 2^-s when the bias joins), so that the lo part of a small
 * weight is a normal fp16 number: at the IDC_FP32 path's distance from the float64 oracle on BOTH weight styles (N = 32: 2.2e-5 torch-default-init,
 * 1.9e-3 full-range, against 2.3e-5 / 1.7e-3; without the scale full-range weights ~0.02 had subnormal lo parts and 3.9e-3), at BF16X3's rate.
 * The price is fp16's range for ACTIVATIONS: beyond +-65504 they saturate (the conversions clamp; nothing becomes inf), below 6e-5 they keep 6e-8 absolute.
 * FP16 (round 6): FP16X3's graph with ONE part and ONE product -- plain fp16 operands (11 significant bits against bf16's 8; unscaled weights), fp32
 * accumulation, every layer on the throughput tiles, the launches on the fp16 twins of the bf16 kernels: 1 / 9 ... 1 / 7 of IDC_BF16's rounding error at
 * 0.96 of its N = 32 rate.  Not a 1e-3 path.
 * The layers of this net are BatchNorm-ed / ReLU-ed activations of O(1..100); a checkpoint with larger activations wants BF16X6. */

/* idc_create flags */
#define IDC_FLAG_DIST_HEAD   0x1u  /* also build model_class (529-bin) head: SIGGRAPHGenerator(dist=True), model.py:105,159-160 */
/* (0x2 reserved: hipGraph replay was left out of the batch-1 path on measurement -- its 51 launches leave < 1 us of gaps
 *  in a 615 us forward, profiles/r02a_click_bf16_trace.txt) */
#define IDC_FLAG_DIST313     0x8u  /* also build the 313-bin distribution / soft-decode head of
                                      models/reference_model/deploy_nopred.prototxt:650-850 (needs the pred.* tensors, see idc_forward_dist313) */
#define IDC_FLAG_GLOBAL_HINTS 0x4u /* also build the Global-Hints branch of models/global_model/deploy_nodist.prototxt:37-172,
                                      501-518 (needs the glob.* tensors, see idc_set_global_hints) */
#define IDC_FLAG_THROUGHPUT_BLOB 0x10u /* weight blob WITHOUT the Winograd images (U = G g G^T of the 3x3 layers and the deconvs).  Since
                                        * round 5 only the fp32 blob carries them (384 MB -> 136 MB with the flag; the direct fp32 kernels then run:
                                        * same results within tolerance, slower); a bf16 blob is 68 MB with or without the flag (round 6; 136 MB in the -DIDC_AB_PARTNERS build, which also carries the layout-2 images) -- the bf16 click
                                        * path's kernels (conv_kwave_*) read the same layout-1 images as the throughput kernels. */

/* ---- library ------------------------------------------------------------------------------- */
int idc_version(void);
/* Process-wide tile-shape policy of the conv kernels (speed only -- every policy computes the same
 * function): 0 automatic (default), 1 small tiles only (conv_igemm), 2 the large-tile bf16 kernel
 * (conv_igemm_v2) wherever it applies.  Exists so that the parity tests can drive every kernel
 * variant at small sizes.  No reference counterpart. */
int idc_set_tile_policy(int policy);
/* Process-wide switches for the parity tests and A/B measurements (speed / kernel choice only: every setting computes the same
 * function).  Eighteen names (round 6: three former environment switches became options; the library reads NO tuning knob from the environment):
 *   "fuse_conv1"  (1)  model1 = conv1_1 + conv1_2 as one launch on the bf16 path; 0 keeps the two launches apart, so that conv1_1's own
 *                      output exists and can be read with idc_get_activation.
 *   "click"       (-1 = on)  small launches (the batch-1 click path, fp32 and what "kwave" does not cover) run conv_click
 *                      (weight tiles by LDS-DMA, fragments prefetched across steps); 0 keeps them on conv_igemm.
 *   "winograd"    (1)  fp32 path: 3x3 stride-1 layers as Winograd F(2x2,3x3), small deconv launches as F(2x2,2x2).  0 = direct kernels,
 *                      1 = automatic, 2 = every deconv too (tests), 12 / 21 / 22 = automatic with the 3x3 form <TB,CB> forced (tests).
 *   "mfma16"      (1)  bf16 throughput tile from v_mfma_f32_16x16x32_bf16 (conv_igemm_v2m / v2p).  0 = conv_igemm_v2 (32x32x16): A/B partner,
 *                      exists only in the -DIDC_AB_PARTNERS build; the default library answers IDC_ERR_UNSUPPORTED.
 *   "v2p"         (1)  the 3x3 convs among them as conv_igemm_v2p (column-swizzled halo tile, unrolled taps; bit-identical to conv_igemm_v2m).
 *   "ds_mfma16"   (1)  deconv + shortcut launches as conv_ds_fused_m, grids with fewer 128-cout workgroups than CUs (model10up of ONE 256x256 image)
 *                      in its 64-cout 4-wave form; 2 = 8-wave workgroups on every grid (A/B, tests); 0 = conv_ds_fused: partner build only.
 *   "split_ds_fuse" (1)  operand-split precisions: each ConvTranspose + the 3x3 shortcut conv it is summed with as ONE launch (conv_ds_fused_ms / _msh:
 *                      both K loops walked per segment into one fp32 accumulator set); 0 = shortcut conv (fp32 sums through HBM) + deconv launch.
 *   "conv1_1_split" (1)  operand-split precisions: conv1_1 (their exact-fp32 island) on conv1_1_split_kernel where the grid is throughput-sized; 0 = conv_igemm<float>.
 *   "conv1_2_split" (1)  ... and conv1_2 (64 -> 64 at full resolution) on conv1_2_split_kernel (conv1_block_fused_t's conv1_2 tile walked per segment); 0 = the generic
 *                      64-cout tile conv_igemm_v2ps<1,4,1>.
 *   "fp16_fast"   (1)  IDC_FP16: launches the bf16 throughput kernels cover run their fp16 twins (conv_igemm_v2ph, conv_ds_fused_mh); 0 = the one-segment
 *                      operand-split kernels everywhere.
 *   "kwave"       (1)  bf16 batch-1 click path: 3x3 stride-1 layers and ConvTranspose launches as conv_kwave_bf16 / conv_kwave_deconv_bf16
 *                      (direct form, K split over the waves of a workgroup); 0 = conv_click + split-K (round 2's kernels).
 *   "kwave_chain" (2)  ... and runs of consecutive same-shape 512-channel layers of that path (conv4_2 .. conv7_3 at batch 1) as ONE
 *                      persistent launch with a grid barrier between layers (conv_kwave_chain_bf16): 0 = one launch per layer,
 *                      1 = through hipLaunchCooperativeKernel, 2 = plain launch after an occupancy check; a workgroup that never sees the
 *                      others gives up after ~0.3 s, that forward fails with IDC_ERR_INTERNAL and the handle goes back to one launch per layer.
 *   "spin_sync"   (1)  calls that serve one or two images wait by polling the stream (bounded) instead of parking on an interrupt; 0 = blocking wait.
 *   "pcie_kernel" (1)  their host <-> device transfers (<= 2 MiB, pinned) run as a copy kernel on the forward's stream; 0 = hipMemcpyAsync.
 *   "op_policy_batch" (0)  single-operator entry points (idc_op_*): the batch the kernel variant is chosen for, as a handle's max_batch is for its
 *                      forwards; 0 = the call's own batch.  The launch always carries the call's batch.  Not read by any forward.
 *   "op_out_f32"  (0)  idc_op_conv2d / idc_op_deconv4x4s2: 1 = the op's output tensor is fp32 in every precision, as the network keeps its class / 313
 *                      logits and hyper-column partial sums, and the kernel is chosen as for such a layer (never the bf16 large tile).
 *                      idc_op_deconv_shortcut then answers IDC_ERR_UNSUPPORTED: the fused launch stores 16-bit outputs only.  Not read by any forward.
 *   "op_resid_f32" (0)  ... 1 = the shortcut sum (resid) of an IDC_BF16 op is an fp32 tensor, as the one a hyper-column launch reads; every other
 *                      precision stores it so already.  Not read by any forward.
 *   "kw_force_abort" (0)  TEST HOOK: 1 makes the persistent trunk launch's first grid barrier unreachable (plays "workgroups never co-resident").
 *   "grid_cap"    (0)  TEST HOOK: v > 0 lowers the grid of every grid-stride launch whose workgroup count is capped (the head, softmax, 313-bin decode,
 *                      colour, ingest, batch, evaluation, audit, split-K epilogue, layout-converter and copy kernels: idc_grid_tag lists them) to at
 *                      most v workgroups, so a small shape makes many passes of the loop.  It never raises a grid above the launcher's own cap and
 *                      changes no result; 0 = off.  Process-wide, takes effect on the next launch; a negative value: IDC_ERR_INVALID_ARG.
 * Retired with their kernels, or folded into the above: "fuse_conv1_small", "winograd_bf16", "winograd_form", "winograd_deconv", "conv1_lw",
 * "code_warm", "kwave_deconv" (IDC_ERR_INVALID_ARG).
 * Take effect on the next forward; unknown names return IDC_ERR_INVALID_ARG. */
int idc_set_option(const char* name, int value);
/* How a call waits for the device (no reference counterpart): calls that serve ONE OR TWO images (the click path) poll the stream instead of
 * blocking in hipStreamSynchronize -- the interrupt wake-up after the copy back costs 15-20 us of a 0.4 ms click -- for a bounded time (a few
 * milliseconds, then they block); batches always block.  IDC_SPIN_SYNC=0 in the environment (read once) restores the blocking wait.
 * The same calls move their transfers of at most 2 MiB between PINNED host memory and the device with a copy kernel on the handle's stream
 * instead of a copy engine (no cross-queue hand-over; IDC_PCIE_KERNEL=0 = hipMemcpyAsync everywhere). */
/* Split-K policy of the small-tile kernels (speed only): 0 automatic (launches too small to fill the chip: the
 * batch-1 click path), 1 never, 2 always (tests).  The slice sums are added in a fixed order: results stay
 * deterministic and independent of how many images a call carries. */
int idc_set_splitk_policy(int policy);
/* Number of visible HIP devices (0 when none; never fails). */
int idc_device_count(void);
/* Text of the last error on this handle (h may be NULL: last error of a failed idc_create or of a
 * handle-less call on the calling thread). */
const char* idc_last_error(idc_handle h);

/* ---- lifetime: replaces SIGGRAPHGenerator.__init__ (model.py:6-132) + net.eval()/.cuda()
 *      in ColorizeImageTorch.prep_net (colorize_image.py:216-233) ---------------------------- */
/* height and width are positive multiples of 8; max_batch has no bound of its own (a tensor of max_batch images may pass 2^31 and 2^32 bytes:
 * images are addressed from 64-bit bases).  The limit is on ONE image: several kernels address one image of a launch's source tensor with 32-bit
 * offsets, and where no kernel is left for some layer of this precision -- its launch ends on the small tile (conv_igemm / conv_click), which reaches
 * 2^31 bytes -- idc_create returns IDC_ERR_INVALID_ARG with the layer, the tensor and its bytes in idc_last_error(NULL), before it asks for a device.
 * Square images: IDC_FP32 up to 2048 x 2048 (conv10_1: H * W * 512 bytes), IDC_BF16 up to 5792 x 5792 (conv9_2, read by the deconv that sums its
 * unfused shortcut: H/2 * W/2 * 256 bytes); the operand-split precisions run every such layer on kernels with 64-bit tile bases. */
int idc_create(int device_id, int height, int width, int max_batch, int precision, unsigned flags,
               idc_handle* out);
int idc_destroy(idc_handle h);

/* Input/output scaling: {l_div, ab_div, mask_mul, out_mul}.  Default = torch backend
 * {100, 110, 1, 110} (model.py:148,175).  The Caffe twin feeds raw values and scales by 100:
 * {1, 1, 1, 100} (colorize_image.py:379-383,425; deploy_nodist.prototxt:812-821).              */
int idc_set_io_scales(idc_handle h, float l_div, float ab_div, float mask_mul, float out_mul);

/* ---- weights: replaces torch.load + load_state_dict (colorize_image.py:222-229) ------------ *
 * Tensors are given under the reference state_dict key names in torch
 * layouts: Conv2d (Cout,Cin,kh,kw); ConvTranspose2d (Cin,Cout,4,4); BatchNorm weight/bias/
 * running_mean/running_var.  Unknown keys (num_batches_tracked, model_class.* without the dist
 * flag) are ignored; a missing key is IDC_ERR_MISSING_KEY.                                      */
typedef struct idc_tensor_desc {
    const char* name;      /* e.g. "model1.0.weight" */
    const float* data;     /* host fp32, C-contiguous */
    int ndim;
    int64_t dims[4];
} idc_tensor_desc;

/* Size of the packed, device-ready weight blob (MFMA-tiled, LDS-swizzled). */
size_t idc_weights_blob_bytes(int precision, unsigned flags);
/* Host-only: pack a state_dict into `blob` (no device needed; used by rank 0 before the RCCL
 * broadcast and by the CPU-side tests). */
int idc_pack_weights(int precision, unsigned flags, const idc_tensor_desc* tensors, int n_tensors,
                     void* blob, size_t blob_bytes);
/* Upload a packed blob from host memory (H2D copy into handle-owned memory). */
int idc_set_weights_host(idc_handle h, const void* blob, size_t blob_bytes);
/* Use a packed blob that already lives in device memory (e.g. a torch uint8 tensor that just
 * received the RCCL broadcast).  copy=0 adopts the pointer (caller keeps it alive), copy=1 does
 * a D2D copy into handle-owned memory. */
int idc_set_weights_device(idc_handle h, const void* dev_blob, size_t blob_bytes, int copy);
/* Convenience = idc_pack_weights + idc_set_weights_host. */
int idc_load_weights(idc_handle h, const idc_tensor_desc* tensors, int n_tensors);
/* Device pointer of the blob in use (NULL before weights are set). */
const void* idc_weights_device_ptr(idc_handle h);

/* ---- forward: replaces SIGGRAPHGenerator.forward (model.py:134-175) ------------------------ *
 * L_mc [n,1,H,W] = L-50; ab [n,2,H,W] raw Lab ab hints (0 where none); mask [n,1,H,W] in {0,1};
 * maskcent = the mask_cent argument (0 or .5, colorize_image.py:210,263).
 * out_ab [n,2,H,W] = 110*tanh(.) -- the tensor the reference returns at colorize_image.py:263.
 * Host-pointer form: blocking; returns when out_ab is valid.  Each pointer that is pinned host memory (idc_alloc_host,
 * hipHostMalloc, hipHostRegister) is transferred in place; pageable ones go through the handle's pinned staging.      */
int idc_forward(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask,
                float maskcent, float* out_ab);
/* Device-pointer form (same layouts, device memory); enqueued on the handle's stream (see STREAM ORDERING at
 * idc_stream: inputs produced / outputs consumed on another stream need idc_stream_wait / idc_stream_signal).
 * sync!=0 waits for completion. */
int idc_forward_device(idc_handle h, int n, const float* d_L_mc, const float* d_ab,
                       const float* d_mask, float maskcent, float* d_out_ab, int sync);
/* dist=True variant (needs IDC_FLAG_DIST_HEAD): additionally writes the 529-bin distribution
 * softmax(0.2*logits) at quarter resolution, dist_q [n,529,H/4,W/4] (the reference's out_cl is
 * its nearest x4 upsample, model.py:160: out_cl[:, :, y, x] == dist_q[:, :, y/4, x/4]).
 * dist_q may be NULL: the distribution then stays resident on the device for idc_dist_at /
 * idc_suggest_colors / idc_get_dist (no 8.7 MB-per-image copy-out on the click path).           */
int idc_forward_dist(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask,
                     float maskcent, float* out_ab, float* dist_q);
/* ---- Global Hints: replaces the glob_ab_313_mask / s_avg_mask inputs of the Caffe global net
 *      (models/global_model/deploy_nodist.prototxt:7-18) as filled by ColorizeImageCaffeGlobDist.net_forward
 *      (colorize_image.py:451-459).  Needs IDC_FLAG_GLOBAL_HINTS.  glob_ab_313_mask [n,314] = 313-bin ab
 *      histogram + 0/1 flag; s_avg_mask [n,2] = mean saturation + flag, or NULL for zeros (the reference
 *      wrapper never fills it).  The values stay in effect for every later forward (images beyond n and a
 *      handle that was never given hints see all-zero inputs -- which is what the reference feeds for
 *      glob_dist == -1: the branch still runs and adds BN(relu(bias)) chains to conv4_3norm).
 *      Weights: 1x1 convs "glob.s_conv1", "glob.glob_conv1" .. "glob.glob_conv4" (.weight (512,Cin,1,1), .bias)
 *      and BatchNorms "glob.bn1" .. "glob.bn4" (weight, bias, running_mean, running_var) -- the Caffe layer
 *      names of the prototxt, in the key style of the converted caffemodel.pth. ----------------------- */
int idc_set_global_hints(idc_handle h, int n, const float* glob_ab_313_mask, const float* s_avg_mask);
int idc_clear_global_hints(idc_handle h);
/* ---- 313-bin distribution head + annealed-mean soft-decode: the Caffe distribution net
 *      models/reference_model/deploy_nopred.prototxt:650-850 as driven by ColorizeImageCaffeDist
 *      (colorize_image.py:466-507).  Needs IDC_FLAG_DIST313.  Hyper-column sum conv3_pred + conv4..7_pred
 *      (ConvTranspose 4x4 s2) + conv8_pred -> ReLU -> pred_313 (1x1, 313 logits at H/4) -> the two grouped
 *      bilinear x2 deconvs (kernel set at colorize_image.py:410-413) -> per full-resolution pixel
 *          dist_S  = softmax(S * logits)                 [n,313,H,W]  (S = 0.2, colorize_image.py:482-485), may be NULL
 *          pred_ab = W_ab . softmax(2.6 * logits) + b_ab [n,2,H,W]    (W_ab = pts_in_hull.T, colorize_image.py:405-407)
 *      out_ab (may be NULL) receives the regression head as in idc_forward.
 *      Weights: "pred.conv3_pred", "pred.conv8_pred" (384,256,3,3); "pred.conv4_pred" .. "pred.conv7_pred"
 *      ConvTranspose (512,384,4,4); "pred.pred_313" (313,384,1,1); "pred.pred_ab" (2,313,1,1) -- .weight/.bias. */
int idc_forward_dist313(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask,
                        float maskcent, float* out_ab, float* pred_ab, float* dist_S);
/* Temperature of dist_S (the reference's scale_S parameter, colorize_image.py:482-485).  Default 0.2. */
int idc_set_dist_temperature(idc_handle h, float S);
/* ---- colour post-processing on the device: replaces lab2rgb_transpose + _set_out_ab_
 *      (colorize_image.py:20-28,196-198,264-267), i.e. skimage.color.lab2rgb / rgb2lab (sRGB, D65, 2 degree
 *      observer), which the reference runs on the host inside every net_forward.
 *      rgb [n,H,W,3] uint8 = (clip(lab2rgb(L, ab), 0, 1) * 255) truncated, exactly the reference expression;
 *      lab_q [n,3,H,W] float64 (may be NULL) = rgb2lab(rgb / 255): the "refreshed" output_lab / output_ab the
 *      reference keeps.  Arithmetic in float64 like skimage.
 *      idc_forward_rgb = idc_forward followed by the post step on the device-resident result, with
 *      L = L_mc + l_cent (l_cent = 50, colorize_image.py:205); out_ab may be NULL. ------------------------- */
int idc_lab2rgb(idc_handle h, int n, const float* L, const float* ab, uint8_t* rgb, double* lab_q);
int idc_forward_rgb(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                    float l_cent, float* out_ab, uint8_t* rgb, double* lab_q);
/*      Round 5 (the reference-API call's host time): of the 2.2 MB idc_forward_rgb sends back per 256x256 click, the value
 *      net_forward RETURNS is the 0.2 MB uint8 image (colorize_image.py:264-268); the ab map (:263) and the refreshed Lab
 *      (_set_out_ab_, :196-198) are attributes a caller may or may not read.  idc_forward_rgb_lazy computes all three on the
 *      device and copies only rgb; idc_fetch_outputs copies the resident ab map (out_ab [n,2,H,W] f32) and / or refreshed Lab
 *      (lab_q [n,3,H,W] f64) of the LAST forward when asked (either may be NULL).  Same values as idc_forward_rgb.
 *      idc_forward_rgb_lazy accepts L_mc == NULL = "the L planes idc_set_image_l left in the handle": the image's L plane does not change
 *      between the clicks on it (colorize_image.py:161-191 sets it in set_image), so the wrapper uploads it once per image. */
int idc_forward_rgb_lazy(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                         float l_cent, uint8_t* rgb);
int idc_fetch_outputs(idc_handle h, int n, float* out_ab, double* lab_q);
/* ---- Global statistics of a reference image: replaces the global_stats.prototxt net the
 *      notebook runs to obtain glob_dist (DemoGlobalHistogramTransfer.ipynb:176-186; models/global_model/
 *      global_stats.prototxt:10-31,101-111,214-244; caffe_traininglayers.py:53-119,161-196; color_quantization.py:7-33):
 *      RGB uint8 -> Lab (skimage rgb2lab) -> 4x4 average pool of ab -> hard 1-nearest-neighbour assignment to the
 *      313 bin centres (NN = 1: weight 1) -> global average = histogram [n,313] (rows sum to 1); s_avg [n] (may be
 *      NULL) = global mean of the HSV saturation (skimage rgb2hsv), the value s_avg_mask would carry.
 *      rgb [n,H,W,3] with the handle's H, W; centres [313,2] = pts_in_hull (a, b). ------------------------------ */
int idc_global_histogram(idc_handle h, int n, const uint8_t* rgb, const float* centres, float* hist, float* s_avg);

/* ---- Click session: the image's L plane and the hint planes stay on the device, a click
 *      sends its rectangle list only.  Replaces the host work in front of every net_forward of the GUI:
 *      UIControl.get_input (ui/ui_control.py:177-187, PointEdit.updateInput :52-63: cv2.rectangle, filled, corners
 *      inclusive, later edits paint over earlier ones, canvas starts black / mask 0) followed by rgb2lab of the
 *      canvas and mask > 0 in gui_draw.compute_result (ui/gui_draw.py:273-277) -- mode IDC_HINT_RGB, c0..c2 = the
 *      uint8 RGB of the edit; or the notebook's put_point (DemoInteractiveColorization.ipynb:131-139) -- mode
 *      IDC_HINT_AB, (c0, c1) = the (a, b) value.  Rectangles are clipped to the image; uncovered pixels get
 *      ab = 0, mask = 0.  mask_value = what a covered mask pixel holds (1; 110 for the Caffe nets' mask_mult).
 *      idc_set_image_l: L_mc [H,W] = L - 50 of image slot img (colorize_image.py:68-77 img_l_mc), uploaded once.
 *      idc_forward_resident: forward of slots 0..n-1 from the resident planes; out_ab [n,2,H,W], rgb [n,H,W,3] u8,
 *      lab_q [n,3,H,W] f64 as in idc_forward_rgb -- each may be NULL.  Handles with a distribution head leave the
 *      distribution resident (idc_keep_dist for the 313 head).  idc_get_hint_planes reads the planes back
 *      (tests; the wrapper's input_ab / input_mask attributes). -------------------------------------------- */
enum { IDC_HINT_AB = 0, IDC_HINT_RGB = 1 };
typedef struct idc_hint { int32_t y0, x0, y1, x1; float c0, c1, c2; } idc_hint;
int idc_set_image_l(idc_handle h, int img, const float* L_mc);
int idc_set_hints(idc_handle h, int img, int n_hints, const idc_hint* hints, int mode, float mask_value);
int idc_get_hint_planes(idc_handle h, int img, float* ab, float* mask);
int idc_forward_resident(idc_handle h, int n, float maskcent, float l_cent, float* out_ab, uint8_t* rgb, double* lab_q);

/* ---- Colour suggestions: ColorizeImageTorchDist.get_ab_reccs (colorize_image.py:322-354)
 *      on the device-resident distribution of the last forward, instead of copying 529 x H x W probabilities to
 *      the host per click.  idc_dist_bins: 529 / 313 / 0.  idc_dist_at: the B probabilities of pixel (y, x) of
 *      image img (the 529 head is stored at H/4: pixel (y/4, x/4), model.py:131,160).  idc_get_dist: the whole
 *      resident tensor ([n,529,H/4,W/4] or [n,313,H,W]).  idc_keep_dist: 313 handles write dist_S on every
 *      forward (82 MB per 256x256 image of device traffic) so that suggestions can follow.
 *      idc_suggest_colors: cmf = cumsum(pdf)/sum (fp32, sequential); N inverse-CDF draws (np.digitize) from the
 *      counter-based generator u_i = lowbias32(i*0x9E3779B9 + seed*0x85EBCA6B + 0x165667B1) >> 8 / 2^24; k-means
 *      with K clusters over the drawn colours centres[bin] ([B,2] = pts_grid / pts_in_hull) -- greedy k-means++
 *      seeding (most-drawn bin, then argmax count x D^2), Lloyd to a fixed point, float64; out_centres [K,2] and
 *      out_conf [K] (= cluster share of the N draws) ordered by occupancy, descending; out_counts [B] (may be
 *      NULL) = draws per bin.  The reference draws from numpy's global RNG and uses sklearn's randomly seeded
 *      KMeans, so its output is not reproducible run to run; this one is a deterministic function of seed. --- */
int idc_dist_bins(idc_handle h);
int idc_keep_dist(idc_handle h, int on);
int idc_dist_at(idc_handle h, int img, int y, int x, float* pdf);
int idc_get_dist(idc_handle h, int n, float* dist);
int idc_suggest_colors(idc_handle h, int img, int y, int x, int K, int N, unsigned seed, const float* centres,
                       double* out_centres, double* out_conf, unsigned* out_counts);
/* ---- Maps of the resident distribution: one streaming pass on the device over what the last forward left there
 *      ([n,529,H/4,W/4] or [n,313,H,W], see idc_get_dist) instead of a copy of it to the host.  Hd x Wd below is
 *      H/4 x W/4 for the 529 head and H x W for the 313 head.
 *      idc_dist_entropy: ent [n,Hd,Wd] = sum_q p log p -- the sign of the reference's compute_entropy
 *      (colorize_image.py:356-357,545-546), i.e. MINUS the entropy -- logf of the stored fp32 p, products and sum in
 *      fp64, rounded to fp32 once.  DEVIATION: a bin with p == 0 contributes 0; the reference's numpy expression
 *      makes that pixel NaN (0 * log 0).
 *      idc_dist_decode: ab [n,2,Hd,Wd] from centres [B,2] (pts_grid / pts_in_hull), conf [n,Hd,Wd] = p_max (may be
 *      NULL).  IDC_DECODE_MODE: the centre of the arg-max bin, equal maxima -> the lowest bin index.
 *      IDC_DECODE_MEAN: w_q = expf(gamma * (logf(p_q) - logf(p_max))), w_q = 0 where p_q == 0;
 *      ab = sum_q w_q c_q / sum_q w_q, sums in fp64.  gamma = 1 is the plain mean; gamma = 2.6 / S on the 313 head
 *      is what pred_ab computes (prototxt :826-850) without its bias.  gamma (checked in both modes) must be
 *      positive and finite.
 *      Both are deterministic, the result for an image does not depend on n, and the distribution is only read.
 *      Status: IDC_ERR_UNSUPPORTED when no distribution is resident (no forward yet, no distribution head, a 313
 *      handle without idc_keep_dist), IDC_ERR_BATCH for n outside 1..(images of the last forward). -------------- */
enum { IDC_DECODE_MODE = 0, IDC_DECODE_MEAN = 1 };
int idc_dist_entropy(idc_handle h, int n, float* ent);
int idc_dist_decode(idc_handle h, int n, int mode, float gamma, const float* centres, float* ab, float* conf);
int idc_sync(idc_handle h);
/* The hipStream_t all work of this handle is enqueued on (as void*): a stream of its own, created non-blocking.
 * STREAM ORDERING: idc_forward_device / idc_forward_resident only ENQUEUE on that stream.  A caller that writes the
 * device inputs or reads the device outputs on another stream (torch's current stream, say) must order the two --
 * either synchronise fully (sync != 0 / idc_sync on this side, a stream/device synchronize on the producer's side),
 * or use the two event helpers below:
 *   idc_stream_wait(h, s)   : work enqueued on the handle AFTER this call waits for everything enqueued on s BEFORE it
 *                             (call it after producing the inputs on s, before idc_forward_device);
 *   idc_stream_signal(h, s) : work enqueued on s AFTER this call waits for everything the handle enqueued BEFORE it
 *                             (call it after idc_forward_device, before consuming d_out_ab on s).
 * The host-pointer entry points (idc_forward, ...) block and need none of this. */
void* idc_stream(idc_handle h);
int idc_stream_wait(idc_handle h, void* caller_stream);
int idc_stream_signal(idc_handle h, void* caller_stream);

/* ---- end-to-end batches: overlapped transfers.  The reference has no counterpart (it
 *      runs one image per call on the host); this is the serving form of idc_forward.  Two slots (0, 1): while slot k
 *      computes, slot 1-k's inputs travel host -> device on a copy stream and its previous result travels back on a third.
 *          idc_forward_async(h, 0, ...batch 0...); idc_forward_async(h, 1, ...batch 1...);
 *          idc_wait(h, 0) -> out of batch 0 valid; idc_forward_async(h, 0, ...batch 2...); idc_wait(h, 1); ...
 *      Host buffers stay caller-owned and must stay untouched until the slot's idc_wait.  Pinned memory (idc_alloc_host,
 *      or the caller's own hipHostMalloc / hipHostRegister) is transferred in place; pageable memory is staged through
 *      pinned buffers with a host memcpy on the calling thread (correct, but the memcpy then bounds the rate).
 *      The blocking entry points drain both slots first.  Each slot owns its device planes: a pipelined batch neither
 *      reads nor replaces the handle's resident L / hint planes or its resident result (idc_forward_resident,
 *      idc_upsample_lab2rgb keep referring to the last BLOCKING forward). */
void* idc_alloc_host(size_t bytes);
int idc_free_host(void* p);
int idc_forward_async(idc_handle h, int slot, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                      float* out_ab);
int idc_wait(idc_handle h, int slot);
/* Where the stages of the slot's last completed batch sat on the device clock: ms6 = milliseconds since the pipeline's
 * first use of {H2D start, H2D end, compute start, compute end, D2H start, D2H end} (HIP events on the three streams).
 * Call after idc_wait(slot).  bench.py's end_to_end leg prints the spans and the overlap achieved, so that a box whose
 * copies do not run under the other slot's kernels shows it (SURVEY.md 8d config 3 "end-to-end").
 * ZERO-COPY alternative (no copy engine involved at all): idc_forward_device accepts PINNED HOST pointers
 * (idc_alloc_host / hipHostMalloc memory is mapped into the device's address space at the same address): conv1's
 * operand staging then reads L / ab / mask over PCIe and the tanh head writes out_ab straight into host memory; the
 * result is valid after idc_sync (or an idc_stream_signal'ed consumer).  Bit-identical to idc_forward. */
int idc_pipeline_times(idc_handle h, int slot, float* ms6);

/* ---- multi-GPU weight distribution (SURVEY.md 8b export list, 8e): one RCCL broadcast of the packed blob over xGMI.
 *      Every rank (one process per GPU) creates its handle; the root also loads the weights.  idc_comm_unique_id
 *      (root only) fills 128 bytes that the caller ships to the other ranks by any side channel (a file, a socket,
 *      torch.distributed's store); then EVERY rank calls idc_broadcast_weights(h, id, rank, world, root).  Non-root
 *      handles receive into their own device allocation, verify header + checksum and become ready.  librccl is
 *      opened on first use -- the copy that ships beside the libamdhip64 this library is bound to (RCCL launches on the
 *      handle's stream, so both must belong to ONE HIP runtime; a process can hold torch's bundled runtime as well);
 *      IDC_ERR_UNSUPPORTED if it cannot be found.  EXPERIMENTAL at world > 1: exercised on hardware with one rank
 *      only (no multi-GPU box was available to the builder); sharded.py's default transport is torch.distributed.  No data-path collective exists: images are
 *      independent (colorize_image.py:232 eval-mode BN), each rank runs its own shard. */
#define IDC_UNIQUE_ID_BYTES 128
int idc_comm_unique_id(void* id128);
int idc_broadcast_weights(idc_handle h, const void* unique_id, int rank, int world, int root);

/* ---- display / full-resolution step on the device: what follows every net_forward in the GUI,
 *          ab_win = cv2.resize(output_ab, (win_w, win_h), interpolation=cv2.INTER_CUBIC)
 *          pred_rgb = (clip(lab2rgb(concat(l_win, ab_win)), 0, 1) * 255).astype('uint8')          ui/gui_draw.py:280-283
 *      and the full-resolution getters get_img_fullres / get_input_img_fullres / get_sup_fullres
 *      (scipy.ndimage.zoom(ab, order=1 | 0) + lab2rgb with img_l_fullres, colorize_image.py:123-158).
 *      source: which resident [2,H,W] ab planes of image slot img -- IDC_SRC_OUTPUT_AB the refreshed (uint8-quantised)
 *      output_ab of the last idc_forward_rgb / idc_forward_resident (float64, what the GUI resizes), IDC_SRC_OUTPUT_AB_RAW
 *      the network's own output, IDC_SRC_INPUT_AB the resident hint planes.  interp: IDC_INTERP_CUBIC = cv2 INTER_CUBIC
 *      (a = -0.75, half-pixel centres, replicated border), IDC_INTERP_LINEAR / IDC_INTERP_NEAREST = scipy zoom order 1 / 0
 *      (corner-aligned).  L [out_h,out_w] float64 = the L channel at the output size (l_win / img_l_fullres);
 *      rgb [out_h,out_w,3] uint8. */
enum { IDC_INTERP_CUBIC = 0, IDC_INTERP_LINEAR = 1, IDC_INTERP_NEAREST = 2 };
enum { IDC_SRC_OUTPUT_AB = 0, IDC_SRC_OUTPUT_AB_RAW = 1, IDC_SRC_INPUT_AB = 2 };
int idc_upsample_lab2rgb(idc_handle h, int img, int source, int interp, int out_h, int out_w, const double* L, uint8_t* rgb);

/* ---- image ingestion on the device: replaces the host work of ColorizeImageBase.load_image / set_image
 *      (colorize_image.py:52-77): cv2.resize(im, (Xd, Xd)) of the uint8 image, rgb2lab of the result, img_l_mc = L - 50.
 *      rgb [n,src_h,src_w,3] uint8 on the host (pinned memory is transferred in place) are the images of slots
 *      img .. img+n-1.  One kernel launch for all n: net-size RGB [H,W,3] by the bilinear rule of cv2 INTER_LINEAR
 *      (half-pixel centres, taps clamped to the image, float64, round half up; the identity when src_h == H and
 *      src_w == W, which is set_image's case: it does not resize), Lab = skimage rgb2lab of that in float64, and the
 *      slot's resident L plane = (float)(L - l_cent) -- what idc_set_image_l would have been given.  rgb_net [n,H,W,3]
 *      uint8 and lab_net [n,3,H,W] float64 receive the net-size image and its Lab; each may be NULL.
 *      IDC_INGEST_KEEP_SOURCE: the source image also stays on the device (src_h*src_w*3 bytes per slot, freed by
 *      idc_destroy or replaced by the slot's next idc_set_image_rgb) for idc_fullres_rgb.  Without the flag the slot's
 *      previous source is released; so it is whenever anything else overwrites the slot's L plane (idc_set_image_l, a
 *      forward that is given L_mc).  Blocking; drains the pipelined slots first.
 *      Status: IDC_ERR_INVALID_ARG for src_h / src_w outside 1..16384, NULL rgb or unknown flag bits; IDC_ERR_BATCH
 *      unless n >= 1 and img + n <= max_batch.
 *      idc_fullres_rgb: the full-resolution getters get_img_fullres / get_input_img_fullres / get_sup_fullres /
 *      get_img_gray_fullres (colorize_image.py:123-158) from the slot's resident source, without the float64 L plane
 *      idc_upsample_lab2rgb is handed: rgb [src_h,src_w,3] uint8 at the source's size.  (a, b): the planes `source` names,
 *      resized by `interp` as in idc_upsample_lab2rgb (same residency rules), or IDC_SRC_NO_AB: a = b = 0.  L: IDC_L_IMAGE
 *      = rgb2lab of the source pixel itself (img_l_fullres), IDC_L_MASK50 = 50 * zoom(mask, order 0) / mask_value with
 *      the slot's resident hint mask and the mask_value of its last idc_set_hints (a slot that never had hints: L = 0).
 *      An output dimension of 1 reads source coordinate 0 on that axis (scipy's zoom).  IDC_ERR_UNSUPPORTED when the
 *      slot has no resident source. */
enum { IDC_INGEST_KEEP_SOURCE = 1 };
int idc_set_image_rgb(idc_handle h, int img, int n, int src_h, int src_w, const uint8_t* rgb, float l_cent, unsigned flags,
                      uint8_t* rgb_net, double* lab_net);
enum { IDC_SRC_NO_AB = 3 };               /* joins IDC_SRC_*: a = b = 0 */
enum { IDC_L_IMAGE = 0, IDC_L_MASK50 = 1 };
int idc_fullres_rgb(idc_handle h, int img, int source, int interp, int l_mode, uint8_t* rgb);

/* ---- edge-aware full-resolution output: joint bilateral ab upsampling (Kopf et al. 2007), guided by the source's own L.  Opt-in: with it
 *      off (the default) no launch and no output byte of any call changes.  The linear zoom above ignores the edges of the full-resolution
 *      L: on a 4x source one net-size pixel of ab is smeared over +-4 source pixels across every object boundary.
 *      THE RULE, for one image: source [h,w,3] uint8; net-size planes a_lo, b_lo [H,W], the planes `source` names, float64 or float32 as
 *      today; net-size guide L_lo[j,i] = (double)Lplane[j,i] + (double)l_cent, where Lplane is the fp32 plane the ingestion wrote for that
 *      image and l_cent is the value it was ingested with; parameters R, sigma_s, sigma_r.  For output pixel (y, x):
 *        L = rgb2lab(source pixel)[0], exactly as IDC_L_IMAGE computes it.
 *        u = (y + 0.5) * ((double)H / h) - 0.5 and v = (x + 0.5) * ((double)W / w) - 0.5: half-pixel centres, the geometry of the ingestion
 *            rule, not the corner-aligned geometry of scipy's zoom.
 *        j0 = (int)floor(u + 0.5) and i0 = (int)floor(v + 0.5).
 *        Taps are j = j0 - R .. j0 + R (outer loop) and i = i0 - R .. i0 + R (inner loop).  A tap outside [0, H) x [0, W) is skipped.
 *        Per tap: ws = exp(-((j - u)^2 + (i - v)^2) / (2 sigma_s^2)); d = L - L_lo[j,i];
 *                 wt = ws * (exp(-(d * d) / (2 sigma_r^2)) + IDC_JOINT_EPS), IDC_JOINT_EPS = 1e-6: where every range weight underflows the
 *                 rule degrades to the spatial Gaussian, not to 0/0;  num_a += wt * a_lo, num_b += wt * b_lo, den += wt.
 *        a = num_a / den and b = num_b / den, then the Lab -> RGB of every other route.
 *      Everything is float64 with fp contract(off).  den > 0 always, because tap (j0, i0) lies inside the image for every h, w >= 1.  (The
 *      kernel computes ws as the product of the two one-dimensional Gaussians, the same value to a few ulp.)
 *      Defaults: R = 2, sigma_s = 1.0 (net-size pixels), sigma_r = 8.0 (L units): plausible values from the literature.  NOBODY HAS
 *      MEASURED THEM ON TRAINED WEIGHTS: this repository has none.
 *      idc_set_joint_upsample: the parameters, handle state.  IDC_ERR_INVALID_ARG unless radius is in 1..4, sigma_s in [0.25, 8] and
 *      sigma_r in [0.5, 100] (a NaN is outside); a refused call changes nothing.
 *      IDC_INTERP_JOINT joins IDC_INTERP_* for idc_fullres_rgb: it needs l_mode == IDC_L_IMAGE, else IDC_ERR_INVALID_ARG; IDC_SRC_NO_AB
 *      stays a = b = 0.  The handle remembers per image slot the l_cent of its last idc_set_image_rgb, and a slot has a resident source only
 *      while that ingestion's L plane is intact, so the guide is defined whenever the call is legal.  idc_upsample_lab2rgb keeps refusing
 *      3: its L is the caller's, it has no guide.
 *      idc_fullres_ab: the interpolated ab map at the source size, ab [2,src_h,src_w] float64, for any of the four interps: what
 *      idc_fullres_rgb feeds to Lab -> RGB.  Same residency rules and statuses as idc_fullres_rgb (NULL ab: IDC_ERR_INVALID_ARG).
 *      idc_set_batch_upsample: IDC_INTERP_LINEAR (default) or IDC_INTERP_JOINT, anything else IDC_ERR_INVALID_ARG.  Handle state, copied
 *      into the slot together with the joint parameters when a pipelined call is enqueued: changing either while a slot is in flight
 *      affects later calls only.  While it is JOINT every source-size output (IDC_BATCH_OUT_SOURCE) of idc_forward_async_rgb, _rgb_ref,
 *      _images, _eval, _dist and _dist_score uses the rule above, guided by the slot's own L plane and the call's l_cent, and is bit for bit
 *      idc_fullres_rgb(IDC_SRC_OUTPUT_AB, IDC_INTERP_JOINT, IDC_L_IMAGE) of the blocking route per image; the sse of an evaluation batch
 *      then scores the joint image. */
enum { IDC_INTERP_JOINT = 3 };            /* joins IDC_INTERP_*: idc_fullres_rgb, idc_fullres_ab, idc_set_batch_upsample */
#define IDC_JOINT_EPS 1e-6
int idc_set_joint_upsample(idc_handle h, int radius, double sigma_s, double sigma_r);
int idc_fullres_ab(idc_handle h, int img, int source, int interp, double* ab);
int idc_set_batch_upsample(idc_handle h, int interp);

/* ---- greyscale sources: single-channel scans in, 8- or 16-bit RGB out (blocking route).  A black-and-white photograph is one plane; an
 *      archive's scan of one has 16 bits.  L passes through this pipeline untouched at the source size (IDC_L_IMAGE), so all 16 bits of
 *      lightness reach the result when the entry and exit formats let them.  There is no expanded RGB copy of the plane on either side.
 *      THE RULE.  Source: one plane [h,w] of uint8 (bits = 8) or uint16 (bits = 16, native byte order, 2-byte-aligned host pointer).  The
 *      pixel's sRGB value is v / 255.0 or v / 65535.0 in float64, the same on all three channels.
 *        Net-size grey: the ingestion rule of idc_set_image_rgb on the one channel (half-pixel centres, taps clamped to the image, float64,
 *            contraction off, round half up), clamped to 0..255 or 0..65535: the 16-bit route rounds on the 16-bit lattice.  The identity
 *            at the net size.
 *        L = rgb2lab's second half on {t, t, t} with t = sRGB-to-linear(value / full scale): the expressions of every other route on those
 *            operands, not a shortened Y-only formula.  The slot's L plane is (float)(L - l_cent).
 *        Source-size output: L of the source sample itself (IDC_L_IMAGE) or IDC_L_MASK50, (a, b) by the interps of idc_fullres_rgb, joint
 *            included, then Lab -> sRGB s in [0, 1] per channel.  8-bit out: (uint8)(s * 255.0), as everywhere.  16-bit out:
 *            (uint16)(s * 65535.0), the same truncation; [.,.,3] uint16, native order.
 *        Two identities follow and the tests hold both.  (I8) a uint8 plane g gives, bit for bit, what the RGB route gives for g repeated
 *            on three channels: the L plane, gray_net == rgb_net[..., 0], l_net == lab_net[:, 0], every image and idc_fullres_ab.  (I16) a
 *            uint16 plane 257 * g gives the results of the uint8 plane g bit for bit where nothing is resized (source size == net size):
 *            fl(257 g / 65535) == fl(g / 255) for every g in 0..255, both the correctly rounded quotient of the same real number.  With a
 *            resize the two differ, because the 16-bit route rounds on the finer lattice: that difference is the point.
 *      idc_set_image_gray = idc_set_image_rgb for n planes pix [n,src_h,src_w]: same slots, same residency rules (IDC_INGEST_KEEP_SOURCE
 *      keeps src_h*src_w*bits/8 bytes per slot), same statuses, and IDC_ERR_INVALID_ARG for bits other than 8 or 16, NULL pix, or an odd
 *      pix / gray_net address at 16 bits.  gray_net [n,H,W] (the sample type) and l_net [n,H,W] float64 receive the net-size plane and
 *      its L; each may be NULL.
 *      A slot's kept source has a format, and every reader of a kept source serves it or refuses it: idc_fullres_rgb serves a grey source
 *      (8-bit out; every source / interp / l_mode it serves for RGB) and so does idc_fullres_ab; idc_reveal_hints and idc_dist_score answer
 *      IDC_ERR_UNSUPPORTED: a grey source has no colour to reveal or to score against.
 *      idc_fullres_rgb16 = idc_fullres_rgb(..., IDC_L_IMAGE) with rgb [src_h,src_w,3] uint16.  IDC_ERR_UNSUPPORTED unless the slot holds a
 *      kept 16-bit grey source; IDC_ERR_INVALID_ARG for a NULL or odd rgb; the codes of idc_fullres_rgb otherwise.
 *      The pipelined form is idc_forward_async_gray, below.  Left out: RGB sources with 16-bit output, a mix of formats within one call,
 *      float sources, ICC profiles and gamma other than sRGB, evaluation and scoring on grey sources. */
int idc_set_image_gray(idc_handle h, int img, int n, int src_h, int src_w, int bits, const void* pix, float l_cent,
                       unsigned flags /* IDC_INGEST_KEEP_SOURCE */, void* gray_net /*[n,H,W] uint8|uint16 or NULL*/,
                       double* l_net /*[n,H,W] or NULL*/);
int idc_fullres_rgb16(idc_handle h, int img, int source, int interp, uint16_t* rgb);   /* kept GRAY16 source, IDC_L_IMAGE */

/* ---- antialiased down-scaling at ingestion: a tent filter stretched by the scale, on the device.  Opt-in: with it off (the default) no
 *      launch, no plan byte and no output byte of any call changes.  The 4-tap rule above point-samples: a 4000 x 3000 scan on a 256 x 256
 *      net uses 4 of every ~180 source samples, and grain, halftone screens and fine texture alias straight into the L plane the network sees.
 *      THE RULE.  One axis has `in` source samples and `out` net samples.  s = (double)in / (double)out.  For output index i:
 *        s <= 1 (same size or up-scaling): today's two clamped taps t0, t1 and weight w of the ingestion rule.  The weights are (1 - w) and w.
 *        s > 1:
 *          c = (i + 0.5) * s
 *          lo = max(0, (int)(c - s + 0.5))
 *          hi = min(in, (int)(c + s + 0.5))
 *          The taps are k = lo .. hi-1.  The window is never empty and holds at most ceil(2 s) + 1 taps: 512 at 16384 -> 64.
 *          r_k = max(0, 1 - |k + 0.5 - c| / s)
 *          tot = sum of r_k in ascending k
 *          weight_k = r_k / tot
 *        This is the tent filter stretched by the scale.  The window is clipped to the image and renormalised, not replicated.  It is the
 *        rule of PIL's BILINEAR resize and of torch's interpolate(mode='bilinear', antialias=True).
 *      Two dimensions, per channel:
 *        t[x] = sum_y wy * f[y][x]: the vertical sum first, ascending y.
 *        v = sum_x wx * t[x], ascending x.
 *        Everything is float64 with contraction off.
 *        The result is floor(v + 0.5) clamped to the source's own lattice: 0..255 for uint8, 0..65535 for uint16.  That is the rounding of
 *        today's rule.
 *      When it applies: to an image only when src_h > H or src_w > W.  An image that is not down-scaled on either axis takes today's
 *      expressions in today's order.  It is then bit-identical to the filter being off.
 *      What follows is unchanged: Lab of the rounded net-size image, L - l_cent into the L plane, hints, the network.  The kept source stays
 *      the original source.  Source-size output takes its L from the original samples exactly as today.
 *      On the device one pre-pass kernel writes the rounded net-size image of every down-scaled image of a call into scratch the handle or
 *      the slot owns, and the ingestion kernels read that image at the net's own size, where their rule is the identity: an image's bits do
 *      not depend on the route, its position or its neighbours.
 *      idc_set_ingest_filter: IDC_FILTER_BILINEAR (default) or IDC_FILTER_ANTIALIAS; anything else is IDC_ERR_INVALID_ARG and changes
 *      nothing.  Handle state.  Like idc_set_batch_upsample, the value is copied into the slot when a pipelined call is enqueued: a batch
 *      in flight keeps what it was enqueued with.  It governs every place the handle brings a source to the net size: idc_set_image_rgb;
 *      idc_set_image_gray, both widths; idc_forward_async_rgb, _rgb_ref, _images, _eval, _dist, _dist_score and _gray; the references of
 *      idc_global_stats_rgb, idc_set_global_refs and of a batch's idc_batch_refs.  Everything that derives from the net-size image follows
 *      it: rgb_net / lab_net / gray_net / l_net, revealed hint colours (idc_reveal_hints on a source kept while the filter was on reads the
 *      image that ingestion made), the net-size truth of sse, the truth of idc_dist_score, the joint upsampling's guide.
 *      Left out: any other filter (box, cubic, Lanczos), antialiasing when up-scaling, the sharded engine, and linear-light averaging: the
 *      filter averages sRGB code values, as every resizer the reference uses does. */
enum { IDC_FILTER_BILINEAR = 0, IDC_FILTER_ANTIALIAS = 1 };
int idc_set_ingest_filter(idc_handle h, int filter);

/* ---- pipelined batches from uint8 images: the serving form of the two calls above on the two slots of idc_forward_async.
 *      rgb_in [n,src_h,src_w,3] uint8 and per-image hint lists in, colourised uint8 images out; idc_wait completes the call and
 *      idc_pipeline_times reports its stages (H2D: the images, the offsets and the hints; compute: the prologue kernel, the
 *      network and the epilogue kernels; D2H: rgb_out and out_ab).  On the device, in one launch each for all n images:
 *      the ingestion rule of idc_set_image_rgb (L - l_cent into the SLOT's L plane) together with the hint rasterisation
 *      of idc_set_hints (image i's hints are hints[hint_offsets[i] .. hint_offsets[i+1]): clipped to the image, corners
 *      inclusive, the later hint wins, uncovered pixels ab = 0 and mask = 0, mode IDC_HINT_AB or IDC_HINT_RGB for the whole
 *      call; hint_offsets == NULL: no image has hints); then the network; then
 *        rgb_out [n,H,W,3]          = what idc_forward_rgb returns for the same L, ab and mask (flags 0), or
 *        rgb_out [n,src_h,src_w,3]  = get_img_fullres (colorize_image.py:123-131) of every image (IDC_BATCH_OUT_SOURCE): the
 *                                     refreshed output_ab zoomed linearly to the source size under the L of the source pixels,
 *                                     what idc_fullres_rgb with IDC_SRC_OUTPUT_AB, IDC_INTERP_LINEAR, IDC_L_IMAGE returns per image.
 *      out_ab [n,2,H,W] receives the network's ab map; it may be NULL.  Bit-identical to the blocking route.
 *      Cost of the hints: every net-size pixel walks its own image's clipped list, last hint first, until one covers it, so
 *      a pixel that no hint covers reads the whole list: n * H * W * (hints per image) steps at worst, in one launch.  That
 *      is meant for the tens of strokes of an editing session; IDC_BATCH_MAX_HINTS is the bound of the argument check, not
 *      a size to serve (2^20 hints on one image of a 32 x 256 x 256 batch are 2e12 steps, seconds of one kernel).
 *      Either entry point may use a slot, in any order.  The slot owns all it needs (source bytes, hint list, planes,
 *      results, pinned staging for pageable callers), grown on demand: like idc_forward_async the call neither reads nor
 *      replaces the handle's resident L / hint planes, kept sources, the mask_value of idc_set_hints or the ab map and
 *      colour results of the last blocking forward.  The distribution heads are not part of this call (idc_forward_async_dist runs them), and the guarantee
 *      does not extend to an IDC_FLAG_DIST313 handle: there every forward through the network, this one included, runs
 *      the 313 head into the handle's pred_ab scratch, and while idc_keep_dist is on it also replaces the resident
 *      distribution, which then belongs to this batch (images 0..n-1).  Without IDC_FLAG_DIST313, or with idc_keep_dist
 *      off, the distribution of the last blocking forward stays resident and readable.
 *      Pinned host buffers are transferred in place; all host buffers stay caller-owned and
 *      untouched until idc_wait (hint_offsets and hints are consumed before the call returns).
 *      Status, all decided on the host before anything is enqueued (a refused call leaves the slot as it was):
 *      IDC_ERR_NO_WEIGHTS before weights are set; IDC_ERR_BATCH for n outside 1..max_batch; IDC_ERR_INVALID_ARG for a slot
 *      outside 0..1 or still in flight, NULL rgb_in or rgb_out, src_h / src_w outside 1..16384, n * src_h * src_w * 3 above
 *      IDC_BATCH_MAX_SOURCE_BYTES, unknown flag bits, a mode that is not 0 or 1, NULL hints while an offset is non-zero,
 *      offsets that do not start at 0, decrease or end beyond IDC_BATCH_MAX_HINTS, an RGB hint colour outside 0..255;
 *      IDC_ERR_UNSUPPORTED while the range audit is on. */
enum { IDC_BATCH_OUT_SOURCE = 1 };
#define IDC_BATCH_MAX_SOURCE_BYTES ((size_t)1 << 30)
#define IDC_BATCH_MAX_HINTS (1 << 20)
int idc_forward_async_rgb(idc_handle h, int slot, int n, int src_h, int src_w, const uint8_t* rgb_in, const int32_t* hint_offsets,
                          const idc_hint* hints, int mode, float mask_value, float maskcent, float l_cent, unsigned flags,
                          uint8_t* rgb_out, float* out_ab);

/* ---- reference-image global hints on the device: "colourise in the palette of a reference photograph" from the photograph's own
 *      uint8 bytes.  Replaces the notebook's get_global_histogram INCLUDING its resize (DemoGlobalHistogramTransfer.ipynb:176-186:
 *      caffe.io.resize_image to the net size, then the global_stats.prototxt net) and the filling of glob_ab_313_mask / s_avg_mask
 *      (colorize_image.py:451-459) -- idc_global_histogram + idc_set_global_hints without the histogram's round trip over the host.
 *      refs [m]: host images [h,w,3] uint8 of INDIVIDUAL sizes (1..16384 a side, IDC_BATCH_MAX_SOURCE_BYTES in all).  Each is sampled to
 *      the handle's H x W by the ingestion rule of idc_set_image_rgb (bilinear, half-pixel centres, clamped taps, float64, round half up;
 *      the identity at h == H and w == W), then idc_global_histogram's statistics: rgb2lab, 4x4 mean of ab in float64, fp32 nearest of the
 *      centres [313,2] (lowest index on a tie), integer counts; and the mean HSV saturation.  A net-size reference gives
 *      idc_global_histogram's histogram bit for bit.  The saturation is summed in a fixed order (no float atomics): every figure of a
 *      reference is bitwise reproducible and depends on nothing but its own pixels and (H, W) -- not on m, not on its neighbours.
 *      DEVIATION: the reference resizes with caffe.io.resize_image (skimage, order 1), which is not runnable here; this is the
 *      project's ingestion rule, the one load_image's replacement uses.  Both are the identity at the net size.
 *      idc_global_stats_rgb: hist [m,313] (rows sum to 1) and s_avg [m] (may be NULL) to the host.  Needs a handle, no weights and no
 *      IDC_FLAG_GLOBAL_HINTS.
 *      idc_set_global_refs: the same statistics written on the device straight into the handle's global inputs of image slots
 *      img .. img+n-1, as the rows idc_set_global_hints would have been given: the histogram, then hist_flag, then -- with
 *      IDC_REF_SATURATION -- {mean saturation, 1}, else {0, 0}.  ref_index [n]: the reference image i takes, -1 = none (an all-zero row:
 *      glob_dist == -1); NULL = the identity (needs m == n).  Rows outside img .. img+n-1 stay as they are (idc_set_global_hints zeroes
 *      them).  Needs IDC_FLAG_GLOBAL_HINTS.
 *      Both calls block: they drain the pipelined slots, enqueue on the handle's stream and return when done.  Beyond what is said
 *      above they touch none of the handle's resident state (L / hint planes, results, distributions, kept sources, the slots).
 *      idc_forward_async_rgb_ref: idc_forward_async_rgb with per-image references, for the same slots, idc_wait and
 *      idc_pipeline_times.  The SLOT owns the packed references, the table, the counts and ITS OWN [max_batch][316] global inputs; the
 *      handle's (idc_set_global_hints / idc_set_global_refs) are neither read nor written, so batch k+1's references travel while batch
 *      k computes.  (idc_forward_async and idc_forward_async_rgb keep reading the handle's.)  On the compute stream, after the slot's
 *      H2D event and in front of the prologue kernel: the counts are zeroed, the statistics kernel, the row kernel; idc_pipeline_times
 *      counts them under compute and the reference bytes under H2D.  m == 0 (refs and ref_index may then be NULL): no image has a
 *      reference, every row is zero.
 *      In all three, refs, ref_index and centres are copied into pinned staging before the call returns: the caller may free them at once.
 *      Status, all decided on the host before anything is enqueued (a refused call leaves slot and handle as they were); for the
 *      arguments idc_forward_async_rgb_ref shares with idc_forward_async_rgb, that call's codes:
 *      IDC_ERR_INVALID_ARG for m outside 1..IDC_REF_MAX (0..IDC_REF_MAX pipelined), NULL refs with m > 0, a NULL refs[r].rgb, h or w
 *      outside 1..16384, reference bytes above IDC_BATCH_MAX_SOURCE_BYTES in all, an index outside -1..m-1, NULL ref_index with
 *      m != n (and m > 0), NULL centres with m > 0, NULL hist in idc_global_stats_rgb, unknown flag bits, a non-finite hist_flag;
 *      IDC_ERR_BATCH unless n >= 1 and img + n <= max_batch; IDC_ERR_UNSUPPORTED for idc_set_global_refs / idc_forward_async_rgb_ref on
 *      a handle without IDC_FLAG_GLOBAL_HINTS.  (The 4x4 blocks need H and W to be multiples of 4: idc_create asks for 8.) */
typedef struct idc_ref_image { const uint8_t* rgb; int32_t h, w; } idc_ref_image;   /* host, [h,w,3] uint8 */
enum { IDC_REF_SATURATION = 1 };
#define IDC_REF_MAX 4096
int idc_global_stats_rgb(idc_handle h, int m, const idc_ref_image* refs, const float* centres, float* hist, float* s_avg);
int idc_set_global_refs(idc_handle h, int img, int n, int m, const idc_ref_image* refs, const int32_t* ref_index,
                        const float* centres, float hist_flag, unsigned flags);
int idc_forward_async_rgb_ref(idc_handle h, int slot, int n, int src_h, int src_w, const uint8_t* rgb_in,
                              const int32_t* hint_offsets, const idc_hint* hints, int mode, float mask_value, float maskcent,
                              float l_cent, unsigned flags, int m, const idc_ref_image* refs, const int32_t* ref_index,
                              const float* centres, float hist_flag, unsigned ref_flags, uint8_t* rgb_out, float* out_ab);

/* ---- pipelined batches of images of INDIVIDUAL sizes: idc_forward_async_rgb / idc_forward_async_rgb_ref for a folder of photographs,
 *      where no two images need share a size.  images [n]: host images [h,w,3] uint8, each with its own pointer and size (1..16384 a
 *      side, IDC_BATCH_MAX_SOURCE_BYTES in all); rgb_out [n]: one host pointer per image.  Image i follows exactly the semantics of
 *      idc_forward_async_rgb called with n = 1 on image i -- ingestion, hints in net coordinates, the network, and
 *        rgb_out[i] [H,W,3]                          (flags 0), or
 *        rgb_out[i] [images[i].h, images[i].w, 3]    (IDC_BATCH_OUT_SOURCE): the full-resolution step under the L of its own source pixels
 *      -- and is bit-identical to it: on the device the images lie packed back to back behind a small table (offset, size and leading
 *      pixel count per image, sent with the hint list), and the prologue and the full-resolution epilogue are still ONE launch each for
 *      all n images.  out_ab [n,2,H,W] or NULL, hint_offsets / hints, mode, mask_value, maskcent, l_cent and flags as in
 *      idc_forward_async_rgb.  refs == NULL: the handle's global inputs are read; otherwise the six reference arguments of
 *      idc_forward_async_rgb_ref, on the slot's own global inputs.  idc_wait and idc_pipeline_times as for the other two calls, and what
 *      is said there about slot ownership, resident state, the 313 head and the range audit applies unchanged.
 *      Host memory: each image pointer, each output pointer and out_ab is judged on its own -- pinned memory is transferred in place,
 *      pageable memory goes through the slot's pinned staging (neighbouring staged images travel as one copy).  images, rgb_out, the
 *      hint arrays and the reference arrays are consumed before the call returns; the image bytes and the output buffers stay the
 *      caller's, untouched, until idc_wait.
 *      Status, all decided on the host before anything is enqueued or any image byte is read (a refused call leaves the slot as it
 *      was): the codes of idc_forward_async_rgb for the shared arguments and, for the reference block, those of
 *      idc_forward_async_rgb_ref; IDC_ERR_INVALID_ARG for NULL images or rgb_out, a NULL images[i].rgb or rgb_out[i], an h or w
 *      outside 1..16384, a sum of source bytes above IDC_BATCH_MAX_SOURCE_BYTES. */
typedef struct idc_batch_refs { int32_t m; const idc_ref_image* refs; const int32_t* ref_index; const float* centres;
                                float hist_flag; uint32_t flags; } idc_batch_refs;   /* as idc_forward_async_rgb_ref's six arguments */
int idc_forward_async_images(idc_handle h, int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets,
                             const idc_hint* hints, int mode, float mask_value, float maskcent, float l_cent, unsigned flags,
                             const idc_batch_refs* refs, uint8_t* const* rgb_out, float* out_ab);

/* ---- evaluation batches: the paper's simulated user and its metric on the device.  The metric is PSNR of the colourised image against the
 *      ground-truth colour image as a function of the number of hints (ColorizeImageBase.get_result_PSNR, data/colorize_image.py:98-108);
 *      the simulated user reveals, per hint, the mean ground-truth ab of the image under the hint's own rectangle (what the notebook's
 *      put_point is fed by hand).  Two device steps around the unchanged forward:
 *        reveal: mode IDC_HINT_REVEAL -- c0..c2 of every rectangle are ignored; its colour is the float64 mean of the image's net-size
 *                (a, b) (idc_set_image_rgb's lab_net) over the clipped rectangle, summed in a fixed order, divided by the pixel count and
 *                rounded once to fp32.  It is a function of the image's bytes, (H, W) and the four clipped corners only.  The list then
 *                goes through the IDC_HINT_AB path unchanged (the later hint wins, clipping, mask_value).  Cost: the rectangle's area per
 *                hint, one workgroup per rectangle;
 *        score:  sse [n,3] = the exact sum over the pixels of image i of (result - truth)^2 per channel (R, G, B) in unsigned 64-bit
 *                integers: the net-size result against the net-size ground truth (idc_set_image_rgb's rgb_net; flags 0), or the
 *                source-size result against the source bytes themselves (IDC_BATCH_OUT_SOURCE).
 *                PSNR = 20 log10(255 / sqrt(sum_c sse / (3 h w))).
 *      idc_reveal_hints (blocking) = idc_set_hints(h, img, n_hints, rects, IDC_HINT_AB, mask_value) with every colour revealed from the
 *      source idc_set_image_rgb kept in slot img (IDC_INGEST_KEEP_SOURCE).  It writes the slot's hint planes and its mask_value and
 *      nothing else of the handle.  colours [n_hints,2] (or NULL) receives the revealed (a, b) of input rectangle k; a rectangle wholly
 *      outside the image receives (0, 0) and paints nothing.  Status: the codes of idc_set_hints; IDC_ERR_UNSUPPORTED when the slot has
 *      no resident source.
 *      idc_forward_async_eval = idc_forward_async_images with mode IDC_HINT_AB / IDC_HINT_RGB (score a given list) or IDC_HINT_REVEAL,
 *      on the same two slots, with idc_wait and idc_pipeline_times: H2D, [reveal], prologue, network, lab_post, [full-resolution
 *      epilogue], score on the compute stream, then sse [n,3] (required), hint_colours [hint_offsets[n],2] (or NULL; IDC_HINT_REVEAL
 *      only; (0, 0) for a dropped rectangle), out_ab [n,2,H,W] (or NULL) and the images (rgb_out == NULL: no image leaves the device)
 *      on the copy-out stream.  Pinned buffers are written in place, pageable ones at idc_wait.  The images and out_ab are bit-identical
 *      to idc_forward_async_images in IDC_HINT_AB mode on the revealed colours.  Slot ownership, resident state, the 313 head and the
 *      range audit: as said for idc_forward_async_images.
 *      Status, all decided before anything is enqueued: the codes of idc_forward_async_images (a NULL rgb_out is allowed here, a NULL
 *      rgb_out[i] in a non-NULL rgb_out is not); IDC_ERR_INVALID_ARG for a NULL sse, a mode outside 0..2, a non-NULL hint_colours with a
 *      mode other than IDC_HINT_REVEAL; the RGB range check applies in IDC_HINT_RGB mode only.
 *      Every other call that takes a hint mode refuses IDC_HINT_REVEAL. */
enum { IDC_HINT_REVEAL = 2 };
int idc_reveal_hints(idc_handle h, int img, int n_hints, const idc_hint* rects, float mask_value, float* colours);
int idc_forward_async_eval(idc_handle h, int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets,
                           const idc_hint* hints, int mode, float mask_value, float maskcent, float l_cent, unsigned flags,
                           const idc_batch_refs* refs, uint8_t* const* rgb_out, float* out_ab, uint64_t* sse, float* hint_colours);

/* ---- distribution batches: where the model is least sure, and what it would suggest there -- for many pixels and many images at once.
 *      The GUI runs the distribution head on every click (ui/gui_draw.py predict_color -> ColorizeImageTorchDist.get_ab_reccs,
 *      data/colorize_image.py:322-354) and shows its entropy map (compute_entropy, :356-357,545-546) for the user to judge where a hint is
 *      needed; the calls below stand in for that judgement and for a loop of get_ab_reccs calls, one pixel each.
 *      Hd x Wd is the distribution's grid as for idc_dist_entropy: H/4 x W/4 (529 head) or H x W (313 head); s = H / Hd.
 *      idc_dist_peaks (blocking; replaces an arg-min search of compute_entropy's map on the host): runs idc_dist_entropy's launch on the
 *      resident distribution of images 0..n-1 and picks, per image, P cells by greedy suppression.  Candidates are the cells whose ent is not
 *      NaN; with IDC_PEAKS_SKIP_HINTS the cells whose s x s block of the handle's resident hint mask (idc_get_hint_planes, as it is at the call)
 *      holds a non-zero value are left out.  For k = 0..P-1: the candidate with the smallest ent (ent is MINUS the entropy: the least certain
 *      cell), ties to the lowest cy * Wd + cx; peaks[i][k] = (cy*s + s/2, cx*s + s/2) in net coordinates and peak_ent[i][k] = its ent; then
 *      every candidate with max(|dy|, |dx|) < radius leaves (radius 1: the cell alone).  With no candidate left: (-1, -1) and +0.0f.  An
 *      image's rows are a function of its own ent and mask values only (not of n; no float atomics; P bounded rounds in one workgroup).
 *      idc_suggest_colors_batch (blocking; replaces nq calls of get_ab_reccs): entry q of out_centres [nq,K,2] / out_conf [nq,K] is bit for bit
 *      what idc_suggest_colors(h, q.img, q.y, q.x, K, N, q.seed, centres, ...) returns, from one upload, one launch (a workgroup per query)
 *      and one copy back.  A query with y == -1 && x == -1 is empty: zeros, nothing read -- the row idc_dist_peaks reports when it ran out.
 *      Both drain the pipelined slots first and only read the distribution.
 *      idc_forward_async_dist (pipelined) = idc_forward_async_eval -- same sixteen arguments, same slots, idc_wait and idc_pipeline_times --
 *      with these differences: all three hint modes are accepted; sse may be NULL (no score) as rgb_out may; the distribution head runs, into
 *      the HANDLE's distribution (d_dist of IDC_FLAG_DIST_HEAD; dist_S of IDC_FLAG_DIST313 with idc_keep_dist on); and after the network the
 *      slot's compute stream runs, in this order, the entropy kernel, the peaks kernel (IDC_PEAKS_SKIP_HINTS reads the SLOT's own mask plane,
 *      the one this batch's hints were rasterised into) and the suggestion kernel.  Their results land in slot-owned device memory and leave on
 *      the copy-out stream: pinned destinations are written in place, pageable ones are filled at idc_wait.  taps->queries name images by their
 *      index in this batch; with IDC_TAPS_SUGGEST_AT_PEAKS (queries must be NULL) the queries are the n * n_peaks peaks in order, read from the
 *      device buffer the picker wrote (no visit to the host), peak (i, k) with seed taps->seed + i * n_peaks + k, and Q = n * n_peaks rows come back.
 *      queries and centres are copied before the call returns.
 *      ORDERING: the distribution is the handle's, not the slot's.  The taps read it on the one compute stream right behind this batch's network
 *      and in front of anything enqueued later, so the other slot's network cannot replace it before they have run; what idc_get_dist /
 *      idc_dist_at / the blocking forms above see after idc_wait is the distribution of the LAST batch enqueued (dist_n = its n), as already
 *      said for IDC_FLAG_DIST313 handles with idc_keep_dist under idc_forward_async_rgb.
 *      Status, all decided on the host before anything is enqueued: for the shared arguments the codes of idc_forward_async_eval;
 *      IDC_ERR_UNSUPPORTED for a handle without a distribution head (neither IDC_FLAG_DIST_HEAD nor IDC_FLAG_DIST313 with idc_keep_dist on), for
 *      the blocking forms without a resident distribution, and while the range audit is on; IDC_ERR_BATCH for n or a query's img outside the
 *      resident images (pipelined: outside this batch); IDC_ERR_INVALID_ARG for NULL taps, P outside 0..IDC_PEAKS_MAX (blocking: 1..), with P > 0
 *      a radius outside 1..max(Hd, Wd), unknown flag bits, NULL peaks with P > 0, IDC_TAPS_SUGGEST_AT_PEAKS with P == 0 or non-NULL queries, a query count
 *      outside 0..IDC_SUGGEST_MAX_QUERIES (blocking: 1..), a query position outside the image that is not the empty query, K or N outside what
 *      idc_suggest_colors accepts, NULL centres or outputs while queries exist. */
enum { IDC_PEAKS_SKIP_HINTS = 1, IDC_TAPS_SUGGEST_AT_PEAKS = 2 };
#define IDC_PEAKS_MAX 256
#define IDC_SUGGEST_MAX_QUERIES 4096
typedef struct idc_dist_query { int32_t img, y, x; uint32_t seed; } idc_dist_query;
int idc_dist_peaks(idc_handle h, int n, int P, int radius, unsigned flags, int32_t* peaks /*[n,P,2]*/, float* peak_ent /*[n,P] or NULL*/);
int idc_suggest_colors_batch(idc_handle h, int nq, const idc_dist_query* q, int K, int N, const float* centres,
                             double* out_centres /*[nq,K,2]*/, double* out_conf /*[nq,K]*/);
typedef struct idc_dist_taps {
    int32_t n_peaks, radius; uint32_t flags;             /* n_peaks 0: no peaks */
    int32_t* peaks; float* peak_ent; float* entropy;     /* [n,P,2]; [n,P] or NULL; [n,Hd,Wd] or NULL */
    int32_t n_queries; const idc_dist_query* queries;    /* img = index in this batch */
    int32_t K, N; uint32_t seed; const float* centres;   /* centres [B,2] */
    double* sugg_centres; double* sugg_conf;             /* [Q,K,2], [Q,K] */
} idc_dist_taps;
int idc_forward_async_dist(idc_handle h, int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets, const idc_hint* hints,
                           int mode, float mask_value, float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs,
                           uint8_t* const* rgb_out, float* out_ab, uint64_t* sse, float* hint_colours, const idc_dist_taps* taps);

/* ---- pipelined batches of greyscale planes: idc_forward_async_images for the sources of idc_set_image_gray (the rule stands there), one
 *      format per call.  images [n]: host planes [h,w] of uint8 (bits 8) or uint16 (bits 16) of INDIVIDUAL sizes; on the device they lie
 *      packed back to back as they came, one or two bytes per pixel.  Image i follows idc_set_image_gray + idc_set_hints +
 *      idc_forward_resident + idc_fullres_rgb / idc_fullres_rgb16 of the blocking route bit for bit:
 *        rgb_out[i] [H,W,3] uint8                      the net-size result (flags 0)
 *        rgb_out[i] [images[i].h, images[i].w, 3] uint8   IDC_BATCH_OUT_SOURCE: L of the source samples, ab by the handle's batch upsample
 *        ... the same as uint16, native order          IDC_BATCH_OUT_SOURCE | IDC_BATCH_OUT_RGB16 (bits 16 only): six bytes a pixel out
 *      out_ab as idc_forward_async_images.  taps != NULL: idc_forward_async_dist without its sse and hint_colours -- peaks, and suggestions
 *      at queries or at the peaks, for a folder of black-and-white photographs (rgb_out may then be NULL: nothing is colourised for the
 *      caller).  Same two slots, idc_wait and idc_pipeline_times; pinned and pageable buffers are told apart per pointer, staged neighbours
 *      travel as one copy.  Everything is decided before anything is enqueued, and a refused call leaves the slot usable.
 *      Status: the codes of idc_forward_async_images (of idc_forward_async_dist with taps) for the shared arguments, and
 *      IDC_ERR_INVALID_ARG for bits not 8 or 16, mode == IDC_HINT_REVEAL, IDC_BATCH_OUT_RGB16 with bits == 8 or without
 *      IDC_BATCH_OUT_SOURCE, an odd pix or rgb_out[i] where the samples are 16-bit, unknown flag bits.  IDC_BATCH_MAX_SOURCE_BYTES bounds
 *      the packed sources and the packed results alike. */
typedef struct idc_gray_image { const void* pix; int32_t h, w; } idc_gray_image;   /* host, [h,w] uint8 or uint16 */
enum { IDC_BATCH_OUT_RGB16 = 2 };          /* joins IDC_BATCH_OUT_SOURCE; idc_forward_async_gray only, bits == 16 only */
int idc_forward_async_gray(idc_handle h, int slot, int n, int bits, const idc_gray_image* images,
                           const int32_t* hint_offsets, const idc_hint* hints, int mode, float mask_value, float maskcent,
                           float l_cent, unsigned flags, const idc_batch_refs* refs, void* const* rgb_out, float* out_ab,
                           const idc_dist_taps* taps /* NULL: no distribution head */);

/* ---- painted hint layers: hints as an RGBA overlay -- scribbles, strokes, polygons, a partly coloured copy of the photograph -- instead of, or
 *      under, a rectangle list.  The rectangle walk costs one comparison per rectangle per pixel; a layer costs its own pixels once.
 *      THE RULE.  A layer is a host image [lh,lw,4] uint8 RGBA with straight alpha, 1..16384 a side, of any size whatever the source's: it is
 *      stretched over the whole image.  alpha_min in 1..255: a layer pixel is PAINTED iff A >= alpha_min.  cover in 0..255.  For cell (y, x) of
 *      the H x W net:
 *        footprint    every layer pixel whose extent overlaps the cell's: rows r0 = (y*lh)/H up to, not including, r1 = ((y+1)*lh + H-1)/H in
 *                     integer arithmetic, columns alike from (x, lw, W).  Never empty; neighbouring footprints share a pixel line when the
 *                     ratio is no integer; a layer smaller than the net gives one pixel to several cells.
 *        counts       tot = the footprint's pixels, cnt = the painted ones.
 *        hinted       iff cnt >= 1 and 255*cnt >= cover*tot, in integers: cover 0 = any painted pixel hints the cell.
 *        colour       the float64 mean over the painted footprint pixels of the (a, b) that IDC_HINT_RGB gives a rectangle of the pixel's
 *                     RGB; alpha does not weight it.  The sum starts at 0.0 and runs in a fixed order, is divided by cnt in float64 and
 *                     rounded once to fp32.  THE ORDER: with bh = the longest row span and bw = the longest column span of the sizes
 *                     (l <= H: 1 if H % l == 0 else 2; l > H: l/H if l % H == 0 else l/H + 2), bh*bw <= 256: row-major upwards through the
 *                     footprint; else 64 partial sums, partial j over the row-major footprint pixels j, j + 64, ... upwards, folded by halves
 *                     (j with j + 32, then + 16, ... + 1).  It depends on (lh, lw, H, W) alone: not on n, the slot, the route or the image's
 *                     place in a batch.
 *        composition  the layer is the canvas the rectangles paint on: a cell covered by any clipped rectangle of the call's list keeps the
 *                     rectangle's value; a cell no rectangle covers and the layer hints gets ab = the mean, mask = mask_value; everything
 *                     else stays ab = 0, mask = 0.  A call that carries a layer needs a finite mask_value != 0.
 *        cells        the exact number of cells the layer hinted after composition, int32 per image.
 *      A net-size layer with cover 0 is therefore, bit for bit, a list of 1 x 1 IDC_HINT_RGB rectangles, one per painted pixel.
 *      idc_set_hints_layer blocks, like idc_set_hints, and with layer == NULL it IS idc_set_hints.  It writes the slot's hint planes and
 *      mask_value and nothing else: idc_get_hint_planes, the full-resolution getters, IDC_PEAKS_SKIP_HINTS and idc_forward_resident see the
 *      result as they see a rectangle list's.  cells (or NULL) receives the one count.
 *      idc_forward_async_layers: idc_forward_async_images (bits 0: images = idc_ref_image[n]) or idc_forward_async_gray without taps (bits 8 |
 *      16: images = idc_gray_image[n]) with a layer per image; with layers == NULL it is that call bit for bit.  layers->layers [n]: rgba NULL
 *      = this image has no layer.  Same two slots, idc_wait and idc_pipeline_times (the layer bytes count under H2D, the kernel under
 *      compute); flags, references, the batch upsample and the ingest filter as in those calls.  The layers travel packed back to back into a
 *      device array of their own: a pinned buffer in place, pageable neighbours staged and sent as one copy.  The layer bytes stay the
 *      caller's until idc_wait; the tables are consumed before return.  An RGBA layer of the source's size is four thirds of the RGB source's
 *      bytes on the bus: a layer may be, and usually should be, smaller than its source.
 *      Status: everything is decided on the host before anything is enqueued, and a refused call leaves the slot and the handle as they
 *      were.  The codes of the calls named above for the shared arguments; IDC_ERR_INVALID_ARG for a layer side outside 1..16384, alpha_min
 *      outside 1..255, cover outside 0..255, a non-NULL layer with NULL rgba in the blocking call, a NULL layers->layers, layer bytes above
 *      IDC_BATCH_MAX_SOURCE_BYTES in all, mask_value zero or not finite while any layer is present, bits not 0, 8 or 16,
 *      mode == IDC_HINT_REVEAL; IDC_ERR_UNSUPPORTED while the range audit is on. */
typedef struct idc_hint_layer { const uint8_t* rgba; int32_t h, w; } idc_hint_layer;      /* rgba NULL: this image has no layer */
typedef struct idc_batch_layers { const idc_hint_layer* layers /*[n]*/; int32_t alpha_min, cover; int32_t* cells /*[n] or NULL*/; } idc_batch_layers;
int idc_set_hints_layer(idc_handle h, int img, int n_hints, const idc_hint* hints, int mode, float mask_value,
                        const idc_hint_layer* layer, int alpha_min, int cover, int32_t* cells);
int idc_forward_async_layers(idc_handle h, int slot, int n, int bits /* 0: idc_ref_image[n] RGB; 8|16: idc_gray_image[n] */, const void* images,
                             const idc_batch_layers* layers, const int32_t* hint_offsets, const idc_hint* hints, int mode, float mask_value,
                             float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs, void* const* rgb_out, float* out_ab);

/* ---- YCbCr 4:2:0 output planes (I420 / NV12): what a JPEG encoder (libjpeg's jpeg_write_raw_data) or a video encoder takes, made on the
 *      device from the uint8 RGB image a call would have returned.  1.5 bytes a pixel leave the device instead of 3, and the host's colour
 *      conversion and chroma subsampling are gone.  Opt-in: with the format IDC_OUT_RGB (the default) no launch, no plan byte and no output byte
 *      of any call changes.
 *      THE RULE, integers only.  Input: the [h,w,3] uint8 RGB image the call would have returned.  The Y plane is [h,w].  The chroma planes are
 *      [ch,cw] with ch = (h + 1) / 2 and cw = (w + 1) / 2; chroma block (j, i) covers rows 2j .. min(2j+1, h-1) and columns 2i .. min(2i+1, w-1):
 *      k = 1, 2 or 4 pixels, clipped at the image's edge, not replicated.
 *        matrices     16.16 fixed point:
 *                       IDC_YCC_JFIF (BT.601, full range; the constants of libjpeg's jccolor.c)
 *                         y = (19595, 38470, 7471)   cb = (-11059, -21709, 32768)   cr = (32768, -27439, -5329)   Yoff = 0
 *                       IDC_YCC_BT709_VIDEO (BT.709, limited range)
 *                         y = (11966, 40254, 4064)   cb = (-6596, -22189, 28785)    cr = (28784, -26145, -2639)   Yoff = 16
 *        per pixel    Y = ((y . (R,G,B) + 32768) >> 16) + Yoff.
 *        per block    S_cb = the sum of cb . (R,G,B) over the block's k pixels; Cb = (S_cb + k * ((128 << 16) + 32767)) >> (16 + log2 k); Cr
 *                     likewise.  The numerator is never negative: the shift is a floor.  For k = 1 this is libjpeg's per-pixel value.
 *        ranges       no clamp exists or is needed: over all 2^24 colours Y, Cb, Cr lie in 0..255 (JFIF) and 16..235 / 16..240 (709), and a block
 *                     mean cannot leave the range of its pixels.
 *        layouts      IDC_OUT_I420: Y, then Cb, then Cr, all row-major without padding: h*w + 2*ch*cw bytes.  IDC_OUT_NV12: Y, then [ch,cw,2]
 *                     with Cb and Cr interleaved: the same byte count.
 *      idc_ycc420_bytes: that count; needs no handle; 0 for h or w outside 1..16384.
 *      idc_set_batch_output: IDC_OUT_RGB (default) / IDC_OUT_I420 / IDC_OUT_NV12 and the matrix; an unknown value of either is
 *      IDC_ERR_INVALID_ARG and changes nothing.  Handle state.  Like idc_set_batch_upsample and idc_set_ingest_filter, the pair is copied into the
 *      slot when a pipelined call is enqueued: a batch in flight keeps what it was enqueued with.  While the format is not IDC_OUT_RGB every
 *      image that idc_forward_async_rgb, _rgb_ref, _images, _eval, _dist, _dist_score, _gray (8-bit result) and _layers return through rgb_out /
 *      rgb_out[i] arrives as that image's plane block, idc_ycc420_bytes(h_i, w_i) bytes in place of the 3 h_i w_i RGB bytes, at the net size and at
 *      the source size (IDC_BATCH_OUT_SOURCE); the same-size calls receive [n][idc_ycc420_bytes(h, w)] back to back.  Everything else a call
 *      returns (out_ab, sse, revealed colours, taps, scores) is unchanged and still derives from the RGB image.  IDC_BATCH_OUT_RGB16 together with
 *      a YCbCr format is IDC_ERR_UNSUPPORTED, decided on the host before anything is enqueued: the slot stays usable.
 *      On the device one post-pass kernel reads the packed RGB results the epilogue wrote and writes the blocks into an array of the slot's own,
 *      which the copy-out stream moves in place of the RGB; idc_pipeline_times counts the kernel under compute.
 *      idc_fullres_ycc = idc_fullres_rgb followed by the conversion: every source, interp (joint included) and l_mode, RGB and grey kept sources,
 *      the codes of idc_fullres_rgb; a NULL out, a format that is not I420 or NV12 (IDC_OUT_RGB included) or an unknown matrix is
 *      IDC_ERR_INVALID_ARG.  out holds idc_ycc420_bytes(src_h, src_w) bytes.
 *      idc_rgb_to_ycc420: the conversion alone on n host images [h,w,3] uint8 of individual sizes, out[i] = image i's block.  Blocking; needs a
 *      handle but no weights; touches none of the handle's resident state.  IDC_ERR_BATCH for n outside 1..IDC_REF_MAX; IDC_ERR_INVALID_ARG for
 *      NULL images / out / images[i].rgb / out[i], a side outside 1..16384, more than IDC_BATCH_MAX_SOURCE_BYTES of RGB in all, an unknown
 *      format (IDC_OUT_RGB included) or matrix.
 *      Left out: 4:2:2 and 4:4:4, 10- and 16-bit planes, other chroma sitings or filters than the clipped box mean, YCbCr sources, the sharded
 *      engine. */
enum { IDC_OUT_RGB = 0, IDC_OUT_I420 = 1, IDC_OUT_NV12 = 2 };
enum { IDC_YCC_JFIF = 0, IDC_YCC_BT709_VIDEO = 1 };
size_t idc_ycc420_bytes(int h, int w);
int idc_set_batch_output(idc_handle h, int format, int matrix);
int idc_fullres_ycc(idc_handle h, int img, int source, int interp, int l_mode, int format, int matrix, uint8_t* out);
int idc_rgb_to_ycc420(idc_handle h, int n, const idc_ref_image* images, int format, int matrix, uint8_t* const* out);

/* ---- frame sequences: a motion-adaptive recursive (temporal) filter on the net-size ab map.  A network of this kind, run frame by frame,
 *      flickers: grain and small exposure changes in L move the ab map by several units between frames of a static shot.  The filter pulls
 *      each pixel's colour towards its own filtered value in the previous frame, strongly where the lightness did not change, not at all
 *      where it did (motion) or where the whole frame changed (a cut).  Opt-in: with it off (the default) no launch, no plan byte and no
 *      output byte of any call changes.
 *      FRAMES are the images of the pipelined calls of one handle, in enqueue order: image 0 .. n-1 of a call, then the next call, whichever
 *      slot it uses.  The handle owns ONE sequence state on the device: y_prev [2,H,W] float32, l_prev [H,W] float32, and whether a frame
 *      has been seen.
 *      THE RULE, for one frame: its fp32 L plane l [H,W] (the slot's plane, (float)(L - l_cent), as ingestion wrote it), the network's fp32
 *      ab map x [2,H,W], the parameters strength s, sigma (L units), radius R, cut c (L units, 0 = never).  Everything is float64 with fp
 *      contract(off).
 *        no previous frame (the first after idc_create or idc_temporal_reset): y = x bit for bit; reported cut = 1, D = 0.
 *        otherwise    e[j,i] = ((double)l[j,i] - (double)l_prev[j,i])^2.
 *                     D = (sum of e over the plane) / (H*W) in float64; the order of the sum is the implementation's own but FIXED: the same
 *                     bits for the same two planes whatever n, slot or position in the call (per 16 x 64 tile: 4 neighbouring pixels per
 *                     thread, a butterfly over the wave, the four waves in order; then the tiles in row-major order).  No float atomics.
 *                     If c > 0 and D > c*c the frame is a scene cut: y = x bit for bit, cut = 1.
 *                     Else m[j,i] = the mean of e over rows j-R .. j+R (outer loop, ascending) and columns i-R .. i+R (inner loop,
 *                     ascending) clipped to the plane: the sum divided by the number of taps inside; nothing is replicated.
 *                     g = s * exp(-m / (2 sigma^2)), and per channel y = (float)((double)x + g * ((double)y_prev - (double)x)).
 *        state        afterwards y_prev <- y (the stored floats, not the float64 values) and l_prev <- l, also after a cut.  Because the
 *                     state is the rounded output, a sequence gives the same bits however it is split into calls.
 *        where y goes y replaces x in the slot's ab map before anything else reads it: the Lab -> RGB epilogue, lab_q, the linear and joint
 *                     source-size kernels, the 16-bit result, the YCbCr post-pass, sse and the returned out_ab all see the filtered map.  The
 *                     distribution heads, their taps and scores, and pred_ab of the 313 head stay on the raw network.
 *      Defaults: strength 0.6, sigma 4.0, radius 1, cut 12.0: plausible values.  NOBODY HAS MEASURED THEM ON TRAINED WEIGHTS: this
 *      repository has none.
 *      idc_set_temporal_filter: handle state, copied into the call when a pipelined call is enqueued, like idc_set_batch_upsample: a batch
 *      in flight keeps what it was enqueued with.  IDC_ERR_INVALID_ARG unless on is 0 or 1, strength in [0, 0.95], sigma in [0.5, 100],
 *      radius in 0..3 and cut 0 or in (0, 100] (a NaN is outside); a refused call changes nothing.  While on it governs
 *      idc_forward_async_rgb, _rgb_ref, _images (with or without references), _eval, _dist, _dist_score, _gray and _layers, at both output
 *      sizes and both depths.  idc_forward_async (the caller's planes) and every blocking forward are not sequences: they neither read nor
 *      advance the state.
 *      idc_temporal_reset: the next frame enqueued starts a sequence.  Ordered behind the batches already enqueued; does not block.
 *      idc_temporal_info: the per-frame cut flags and D of the slot's last completed call; they travel back with the call's small results.
 *      IDC_ERR_INVALID_ARG for a slot outside 0..1, both pointers NULL, a slot still in flight, or a slot whose last call ran with the
 *      filter off (or that never ran), in this order.
 *      idc_temporal_apply: the rule alone on host arrays ab [n,2,H,W], l [n,H,W] -> y [n,2,H,W] (cut [n], D [n] may be NULL), through the same
 *      kernels; it reads and advances the handle's state with the handle's current parameters.  Blocks, drains the slots first, needs no
 *      weights, runs whether `on` is set or not.  IDC_ERR_BATCH for n outside 1..max_batch; IDC_ERR_INVALID_ARG for a NULL ab, l or y.
 *      idc_temporal_state: the state as it stands behind everything enqueued: y_prev [2,H,W], l_prev [H,W] (zeros while have is 0), have;
 *      each pointer may be NULL.  Blocks.
 *      Status: everything is decided on the host before anything is enqueued, and a call refused there leaves the state as it was.  The
 *      pipelined calls keep their own tables; the filter adds no row to them.  A call that fails LATER, with IDC_ERR_HIP from the runtime
 *      while it is being enqueued, may already have advanced the sequence: idc_temporal_reset before going on.
 *      Left out: more than one sequence per handle, the blocking routes, the sharded engine, filtering the distribution or pred_ab, a raw
 *      out_ab beside the filtered one (the filter-off call gives it).  Motion compensation: the next section.
 *
 *      MOTION COMPENSATION of that filter (idc_set_temporal_motion).  The rule above lets go wherever L changed, by design -- and so on
 *      everything that moves and on every pixel of a pan, where flicker shows most.  With motion on, the previous state is first warped along
 *      block-matched vectors, so a moving surface is compared with, and pulled towards, ITSELF in the previous frame.  Opt-in, off by
 *      default: with it off no launch, plan byte or output byte of any call changes.  Everything is at the net size, on the L planes the slots
 *      already hold.
 *      THE RULE, for a frame with a predecessor: its L plane l [H,W] float32, the state l_prev, y_prev, the network's x, search S in 0..7,
 *      penalty lambda (L^2 per squared pixel of displacement).  H and W are multiples of 8 (idc_create).  All arithmetic is float64 with fp
 *      contract(off).
 *        blocks       8 x 8: block (by, bx) covers rows 8by .. 8by+7 and columns 8bx .. 8bx+7.
 *        candidates   every (dy, dx) in [-S, S]^2, RANKED by (dy^2 + dx^2, dy, dx) ascending, so rank 0 is (0, 0).  A candidate is valid for a
 *                     block iff the displaced block lies wholly inside the plane; nothing is replicated.  (0, 0) is always valid.
 *        cost         C = sum over r = 0..7 (outer, ascending), c = 0..7 (inner, ascending) of
 *                     ((double)l[8by+r, 8bx+c] - (double)l_prev[8by+r+dy, 8bx+c+dx])^2, with ONE accumulator starting at +0;
 *                     J = C / 64 + lambda * (double)(dy^2 + dx^2).  The order is normative: J has the same bits in every implementation.
 *        choice       best starts as rank 0; a later valid candidate replaces it iff its J < best strictly: ties go to the lower rank, a NaN
 *                     never wins.  A parallel reduction over (J, rank) pairs is the same function.  v[by,bx] = (dy, dx) as int8.
 *        warp         for every pixel p of the block: lw[p] = l_prev[p + v] and yw[ch][p] = y_prev[ch][p + v].
 *        filter       the rule above, unchanged, with lw in place of l_prev and yw in place of y_prev: e, then D summed in the SAME fixed order
 *                     as the plain rule (at S = 0 its bits are the plain rule's), so the cut test is on the compensated difference and a pan
 *                     is no cut; the window mean m crosses block borders and takes each pixel's own e; then g and y.
 *        state        afterwards y_prev <- y and l_prev <- l (UNWARPED), also after a cut.
 *        no predecessor: y = x, and v is reported as zeros.  A cut frame: y = x, and the vectors are reported as estimated.
 *      Defaults: search 4, penalty 0.5: plausible values.  NOBODY HAS MEASURED THEM ON TRAINED WEIGHTS: this repository has none.
 *      idc_set_temporal_motion: handle state, copied into a pipelined call when it is enqueued, like idc_set_temporal_filter.
 *      IDC_ERR_INVALID_ARG unless on is 0 or 1, search in 0..7 and penalty in [0, 1e6] (a NaN is outside); a refused call changes nothing.  It
 *      acts only where the temporal filter acts -- the eight pipelined entry points and idc_temporal_apply, which uses the handle's current
 *      setting -- and with the temporal filter off it does nothing.
 *      idc_temporal_vectors: v int8 [n, H/8, W/8, 2] (dy, dx).  slot 0..1: of the slot's last completed call; the vectors travel back with the
 *      call's small results, and only when motion was on.  slot -1: of the last idc_temporal_apply.  IDC_ERR_INVALID_ARG for a slot outside
 *      -1..1, a NULL v, a slot still in flight, a slot whose last call ran with the filter off (or that never ran; slot -1: no
 *      idc_temporal_apply yet), or a call that ran without motion, in this order.
 *      Left out: sub-pixel vectors, a hierarchical or wider search, smoothing or a median of the vector field, overlapped-block compensation,
 *      occlusion handling beyond what e already does, more than one sequence per handle, the blocking routes and wrapper classes, the
 *      sharded engine, tuning the defaults on trained weights.  Hints that follow the vectors: the next section (HINT TRACKING).
 *
 *      HINT TRACKING along those vectors (idc_set_hint_tracking).  Hints are an input of the network, and the vectors of a call's frames
 *      exist only once the call runs: without tracking a click made on a coat stays at its net coordinates and is on the wall a dozen frames
 *      into a pan.  With tracking on, the search runs in FRONT of the network (it reads the L planes alone) and the hint planes are carried
 *      along its vectors on the device, so every frame of a batch gets its tracked hints in the same call.  Opt-in, off by default: with it
 *      off no launch, plan byte or output byte of any call changes.
 *      Parameters: life, an integer in 0..65535 (frames a hint may be carried; 0: no limit); tol, L units in [0, 100].
 *      Defaults: life 0, tol 8.0: plausible values.  NOBODY HAS MEASURED THEM ON TRAINED WEIGHTS: this repository has none.
 *      Tracking acts only where motion compensation acts: the eight pipelined entry points, enqueued with the temporal filter on AND motion
 *      on.  Otherwise it does nothing.
 *      THE RULE, for frame f of the sequence.  Its OWN planes ab_f [2,H,W] and mask_f [H,W] are what the untouched prologue wrote for this
 *      frame (with the hint-layer kernel where the call has layers, and the revealed colours in an evaluation call); l_f is its fp32 L plane;
 *      v_f are exactly the motion rule's vectors, estimated against the predecessor's L.  The TRACKED planes (A_f, M_f, G_f) hold ab, mask
 *      and an int32 age.
 *        own          where mask_f[p] != 0: A_f[p] = ab_f[p], M_f[p] = mask_f[p], G_f[p] = 0.  An own hint always wins.
 *        carried      elsewhere, with a predecessor: q = p + v_f[p.y / 8, p.x / 8] (always inside the plane: a valid vector keeps its whole
 *                     block inside).  The hint is carried iff M_{f-1}[q] != 0, and fabs((double)l_f[p] - (double)l_{f-1}[q]) <= tol (a NaN
 *                     carries nothing), and life == 0 || G_{f-1}[q] + 1 <= life.  Then A_f[p] = A_{f-1}[q] and M_f[p] = M_{f-1}[q] -- the
 *                     stored floats, so the origin call's mask_value travels with the hint -- and G_f[p] = G_{f-1}[q] + 1 (it stops at
 *                     2^31 - 1).  Otherwise (0, 0, 0, 0) is written.
 *        no predecessor (the first frame after idc_create or idc_temporal_reset): tracked = own.
 *        state        the handle keeps (A, M, G) of the sequence's last frame beside y_prev / l_prev; idc_temporal_reset clears it.  A
 *                     pipelined call enqueued with the filter on but tracking off, or with motion off, DROPS it (and so does
 *                     idc_temporal_apply, which moves l_prev on without hints): the next tracking call's frame 0 then carries nothing.  A
 *                     filter-off call, idc_forward_async and the blocking forwards leave it alone.  The state is the stored planes, so a
 *                     sequence gives the same bits however it is split into calls.
 *      The tracked planes replace the own planes before anything else reads them: the network, skip_hints of the uncertainty peaks, the
 *      taps.  Revealed colours, `cells` of a layer call and idc_temporal_info are unchanged.  The filter's cut test is not consulted: a cut
 *      ends the carried hints through tol, pixel by pixel.
 *      idc_set_hint_tracking: handle state, copied into a pipelined call when it is enqueued, like idc_set_temporal_motion.
 *      IDC_ERR_INVALID_ARG unless on is 0 or 1, life in 0..65535 and tol in [0, 100] (a NaN is outside); a refused call changes nothing.
 *      idc_tracked_hints: the tracked planes of the slot's last completed call; each pointer may be NULL, not all three.  It copies from the
 *      device on request only: nothing is added to a call's own D2H traffic.  IDC_ERR_INVALID_ARG for a slot outside 0..1, all pointers
 *      NULL, a slot still in flight, a slot whose last call ran with the filter off (or that never ran), or a call that ran without
 *      tracking, in this order.
 *      idc_track_hints_apply: the rule alone on host arrays, through the same search and tracking kernels, with the handle's current motion
 *      (search, penalty) and tracking (life, tol) parameters, as a self-contained sequence: frame 0 has no predecessor, and the handle's
 *      sequence state is neither read nor written.  It blocks, drains the slots and needs no weights.  IDC_ERR_BATCH for n outside
 *      1..max_batch, IDC_ERR_INVALID_ARG for a NULL input or output plane; v_out [n, H/8, W/8, 2] may be NULL.
 *      Left out: dropping carried hints at a key frame, sub-block vectors, forward or bidirectional tracking, the blocking routes, the
 *      sharded engine, tuning the defaults. */
int idc_set_temporal_filter(idc_handle h, int on, double strength, double sigma, int radius, double cut);
int idc_set_temporal_motion(idc_handle h, int on, int search, double penalty);
int idc_temporal_vectors(idc_handle h, int slot, int8_t* v /*[n, H/8, W/8, 2] (dy, dx)*/);
int idc_set_hint_tracking(idc_handle h, int on, int life, double tol);
int idc_tracked_hints(idc_handle h, int slot, float* ab /*[n,2,H,W]*/, float* mask /*[n,H,W]*/, int32_t* age /*[n,H,W]*/);
int idc_track_hints_apply(idc_handle h, int n, const float* l /*[n,H,W]*/, const float* ab /*[n,2,H,W]*/, const float* mask /*[n,H,W]*/,
                          float* ab_out /*[n,2,H,W]*/, float* mask_out /*[n,H,W]*/, int32_t* age_out /*[n,H,W]*/,
                          int8_t* v_out /*[n, H/8, W/8, 2] or NULL*/);
int idc_temporal_reset(idc_handle h);
int idc_temporal_info(idc_handle h, int slot, int32_t* cut /*[n]*/, double* D /*[n]*/);
int idc_temporal_apply(idc_handle h, int n, const float* ab /*[n,2,H,W]*/, const float* l /*[n,H,W]*/, float* y /*[n,2,H,W]*/,
                       int32_t* cut /*[n] or NULL*/, double* D /*[n] or NULL*/);
int idc_temporal_state(idc_handle h, float* y_prev /*[2,H,W]*/, float* l_prev /*[H,W]*/, int32_t* have);

/* ---- distribution scores: how much probability did the head put on the colour the pixel really has?  The question the distribution heads
 *      were trained on: the reference's training layers encode the ground-truth ab into the colour bins with NNEncode
 *      (caffe_files/color_quantization.py:7-33; NNEncLayer: NN = 1, sigma = 5, NN = 10 commented beside it, caffe_traininglayers.py:161-189) and
 *      feed a softmax cross-entropy.  Scored on the device from the resident distribution and the ground-truth image's own bytes, instead of
 *      idc_get_dist (82 MB per 256x256 image on the 313 head), a host rgb2lab and a nearest-neighbour search and a sort per cell.
 *      Hd x Wd is the distribution's grid as for idc_dist_entropy, s = H / Hd (4: 529 head, 1: 313 head), B the bin count, centres [B,2] fp32
 *      (a, b) as in idc_suggest_colors.  For image i and cell (cy, cx):
 *        1. truth (a*, b*) fp32 = the colour idc_reveal_hints reports for the rectangle (cy*s, cx*s, cy*s+s-1, cx*s+s-1) of that image, bit for
 *           bit: the same device functions per net-size pixel (bilinear_taps, bilinear_q, linear_to_lab), the float64 sum in
 *           reveal_hints_kernel's order for a 16-pixel rectangle -- pixel t = dy*4+dx, folded by halves (t with t+8, then +4, +2, +1) -- divided
 *           by the count in float64 and rounded once to fp32; for s = 1 the pixel's own (a, b) rounded to fp32.
 *        2. neighbours q_1 .. q_nn = the nn centres nearest to the truth in Euclidean distance, computed in float64 from the fp32 values
 *           (d^2 = da*da + db*db, no fused multiply-add), ascending, ties to the lower index; t = q_1 is the target bin; nn in 1..16.  (The
 *           device orders by d^2, which orders as d does except where two different d^2 round to one square root.)
 *        3. weights w_j = exp(-d_j^2 / (2 sigma^2)) / sum_k exp(-d_k^2 / (2 sigma^2)) in float64, the sum with k ascending
 *           (NNEncode.encode_points_mtx_nd); exactly 1 for nn == 1.  (A sigma so small that every term underflows gives NaN, as there.)
 *        4. xent of the cell = 0 - sum_j w_j * log(max(p[q_j], FLT_MIN)): p the stored fp32 probability, float64 log, products and sum, j
 *           ascending.  The floor is Caffe's softmax-loss rule: a zero probability gives a large finite value, not inf.
 *        5. rank of the cell = the number of bins q with p[q] > p[t] || (p[q] == p[t] && q < t): int32 in 0..B-1, 0 = the head's most probable
 *           bin is the true one.
 *        6. hits[i][j] = the number of cells of image i with rank < ranks[j], up to 8 thresholds in 1..B: uint32, exact (integer atomics).
 *        7. xent[i] = the float64 sum of the image's cell values in this FIXED order (no float atomics): the cells c = cy*Wd + cx in blocks of 64
 *           consecutive cells (the last block padded with +0.0), each block folded by halves (c with c+32, then +16, +8, +4, +2, +1); then 64
 *           running sums, sum l taking the block sums l, l+64, l+128, ... in ascending order starting from +0.0, folded by halves in the same
 *           way.  A function of the image's own cells only -- not of n, the slot or timing.  The mean is xent[i] / (Hd*Wd): the host divides.
 *      idc_dist_score (blocking) scores the resident distribution of images 0..n-1 against the sources idc_set_image_rgb(...,
 *      IDC_INGEST_KEEP_SOURCE) kept in slots 0..n-1 (idc_reveal_hints' rule).  It drains the pipelined slots first, reads the distribution and the
 *      sources and writes nothing of the handle's resident state.
 *      idc_forward_async_dist_score = idc_forward_async_dist (its seventeen arguments first) with the score as one more tap on the slot's compute
 *      stream, behind the batch's network and behind the other taps: that call's ORDERING paragraph applies unchanged.  The ground truth is the
 *      slot's own packed source images.  Results land in slot-owned device memory and leave on the copy-out stream: pinned destinations are
 *      written in place, pageable ones are filled at idc_wait.  taps may be NULL here: then only the score runs.  spec and centres are copied
 *      before the call returns.
 *      Status, all decided on the host before anything is enqueued (a refused call leaves slot and handle as they were): for the shared arguments
 *      the codes of idc_forward_async_dist; IDC_ERR_UNSUPPORTED on a handle without a distribution head, for the blocking form without a resident
 *      distribution or when one of its slots has no kept source, and while the range audit is on; IDC_ERR_INVALID_ARG for a NULL spec, out,
 *      out->xent or centres, nn outside 1..min(16, B), a sigma that is not finite and > 0, n_ranks outside 0..8, a threshold outside 1..B, NULL
 *      hits with n_ranks > 0; IDC_ERR_BATCH for n outside the resident images.
 *      Not here: the class-rebalancing / prior-boost weights of the training layers. */
#define IDC_SCORE_MAX_NN 16
#define IDC_SCORE_MAX_RANKS 8
typedef struct idc_dist_score_spec { int32_t nn; float sigma; int32_t n_ranks; int32_t ranks[8]; } idc_dist_score_spec;
typedef struct idc_dist_score_out {      /* every pointer may be NULL except xent */
    double* xent;      /* [n] */            uint32_t* hits;    /* [n,n_ranks] */
    double* xent_map;  /* [n,Hd,Wd] */      int32_t* rank_map; /* [n,Hd,Wd] */
    int32_t* target;   /* [n,Hd,Wd] */      float* truth_ab;   /* [n,2,Hd,Wd] */
} idc_dist_score_out;
int idc_dist_score(idc_handle h, int n, const idc_dist_score_spec* spec, const float* centres, const idc_dist_score_out* out);
int idc_forward_async_dist_score(idc_handle h, int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets, const idc_hint* hints,
                                 int mode, float mask_value, float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs,
                                 uint8_t* const* rgb_out, float* out_ab, uint64_t* sse, float* hint_colours, const idc_dist_taps* taps,
                                 const idc_dist_score_spec* spec, const float* centres, const idc_dist_score_out* out);

/* ---- colour picker on the device: replaces data/lab_gamut.py, the host colour maths the GUI runs on every mouse press
 *      (ui/gui_draw.py:11,182-183,195-204; ui/gui_gamut.py:4), in float64 with the constants and operation order of idc_lab2rgb.
 *      idc_gamut_map = abGrid(gamut_size, D).update_gamut(L[k]) (lab_gamut.py:56-78) for k = 0..n-1 in one launch.  The grid has
 *      side A = B = len(arange(-gamut_size, gamut_size + D, D)) = ceil(2 gamut_size / D) + 1; point (i, j) is (a, b) =
 *      (-gamut_size + i D, -gamut_size + j D): the row is a, the column b (:58-60).  Per point
 *          pts_rgb    = (255 * clip(lab2rgb(L, a, b), 0, 1)) truncated to uint8                                       (:70)
 *          mask       = |(L, a, b) - rgb2lab(pts_rgb / 255)|_2 < 1.0, strictly                                       (:71-74)
 *          masked_rgb = mask ? pts_rgb : 255                                                                         (:75-77)
 *      pts_rgb / masked_rgb [n,A,B,3] uint8, mask [n,A,B] uint8 in {0,1}; each may be NULL, not all three.
 *      idc_snap_colors = snap_ab(L[k], rgb[k]) (lab_gamut.py:28-52) for n colours in one launch: Lab of the colour, then up to 20
 *      rounds of "L := L[k]; lab -> clip(rgb, 0, 1) -> lab" on the UNQUANTISED sRGB triple, ending after the first round whose
 *      sum |delta lab| < 1.  As in the reference, the Lab value that leaves the loop carries the round-tripped L, not L[k] (:36-40).
 *          rgb_out [n,3] uint8  = round-half-even(clip(lab2rgb(that Lab), 0, 1) * 255)     return_type 'rgb'         (:46, :24)
 *          lab_out [n,3] f64    = rgb2lab(rgb_out / 255)                                   return_type 'lab'         (:51)
 *          iters   [n]   int32  = rounds run, 1..20 (no reference counterpart: tells a knife-edge case from a wrong formula)
 *      each may be NULL, not all three.  rgb [n,3] uint8.
 *      Both need a handle but no weights, enqueue on the handle's stream and block until the result is on the host.  They neither read
 *      nor write the handle's resident state (L / hint planes, the last forward's maps and distribution, kept sources, the pipelined
 *      slots); their staging buffers grow on demand and are freed by idc_destroy.
 *      Status: IDC_ERR_INVALID_ARG for n < 1, n > 64 maps / n > 65536 colours, a NULL input, a non-finite L (checked on the host before
 *      anything is launched), gamut_size outside 1..512, D outside 1..gamut_size, or every output NULL. */
#define IDC_GAMUT_MAX_MAPS 64
#define IDC_GAMUT_MAX_SIZE 512
#define IDC_SNAP_MAX_COLORS 65536
int idc_gamut_map(idc_handle h, int n, const double* L, int gamut_size, int D, uint8_t* pts_rgb, uint8_t* masked_rgb, uint8_t* mask);
int idc_snap_colors(idc_handle h, int n, const double* L, const uint8_t* rgb, uint8_t* rgb_out, double* lab_out, int32_t* iters);

/* ---- introspection for parity tests and roofline accounting -------------------------------- */
int idc_num_layers(idc_handle h);
typedef struct idc_layer_info {
    char name[32];        /* caffe-style layer name: conv1_1 ... conv10_2, conv3_3_short, head ... */
    char kernel[48];      /* kernel family launched */
    double flops;         /* ALGORITHMIC flops per image (2*MACs), 0 for non-conv */
    double min_bytes;     /* algorithmic HBM bytes per image: input + output + residual (+weights once) */
    int launches;         /* kernel launches per forward */
} idc_layer_info;
int idc_layer_info_get(idc_handle h, int layer, idc_layer_info* out);
/* Per-layer timing with hipEvents on the handle's stream.  While on, every forward records an
 * event pair around each layer (kept for the last 32 forwards); idc_layer_times_ms() syncs and
 * returns, for layers [0, idc_num_layers), the mean duration (ms) over the forwards recorded
 * since profiling was switched on (at most the last 32). */
/* on = 2: a single event pair around the whole forward instead (ms[0] of idc_layer_times_ms = mean forward duration,
 * the other entries 0) -- the per-launch pairs of mode 1 slow a batch-32 forward by about 4 %. */
int idc_set_profiling(idc_handle h, int on);
int idc_layer_times_ms(idc_handle h, float* ms, int capacity);
/* The same recorded forwards as per-layer min / median / max (ms) instead of the mean: tells a layer that is slow on every forward
 * from one that was slow once (first launch of a kernel variant, a clock step) -- bench.py's `layers_ms` is the median of 20. */
int idc_layer_times_stats(idc_handle h, float* ms_min, float* ms_median, float* ms_max, int capacity);
/* Copy an intermediate activation of the LAST forward to the host as NCHW fp32.
 * name = idc_layer_info.name; out must hold n*C*H*W floats; *C,*H,*W are returned.            */
int idc_get_activation(idc_handle h, const char* name, int n, float* out, size_t capacity_floats,
                       int* C, int* H, int* W);

/* ---- range audit: does this checkpoint fit the storage format of this precision? ----------- *
 * The fp16 forms (IDC_FP16X3, IDC_FP16) clamp every stored activation to +-65504 and keep only a subnormal's absolute precision below 2^-14,
 * silently.  While the audit is on, every forward (blocking, resident and device-pointer forms; the pipelined slots answer
 * IDC_ERR_UNSUPPORTED) runs one streaming reduction over each layer's STORED output right after the layer's launch -- the values the next layer
 * reads: scaled by 2^act_exp on a handle loaded with activation exponents, the sum of the parts for the operand-split forms -- and folds it
 * into a per-layer record that is sticky across forwards (max of maxima, sums of counts) until the reset call.  The forward's results do not
 * change by a bit.  The report call synchronises the stream; `layer` indexes the table of idc_layer_info_get.  Layers without a stored output
 * of their own in the current plan (conv1_1 inside the fused conv1 block, a shortcut conv inside the fused deconv launch, conv10_2 when the
 * head rides in its epilogue) and the non-conv rows report n_values = 0. */
enum { IDC_STORE_NONE = 0, IDC_STORE_F32 = 1, IDC_STORE_BF16 = 2, IDC_STORE_F16 = 3 };
typedef struct idc_range_info {
    char name[32];           /* idc_layer_info.name */
    int storage;             /* IDC_STORE_*: element type of the stored tensor */
    int parts;               /* planes per pixel whose sum is the value (1; 2 / 3 for the operand-split precisions) */
    int act_exp;             /* the stored tensor holds value * 2^act_exp (0 unless the weights were loaded with exponents) */
    float max_abs;           /* over the finite stored values */
    uint64_t n_values;       /* n * cout * h * w, summed over the audited forwards */
    uint64_t n_saturated;    /* |value| >= 65504 in an fp16 storage form (0 for bf16 / fp32 storage) */
    uint64_t n_tiny;         /* non-zero and |value| < 2^-14: the hi part itself would be subnormal in fp16 */
    uint64_t n_nonfinite;    /* NaN / inf (not part of max_abs) */
} idc_range_info;
int idc_set_range_audit(idc_handle h, int on);
int idc_range_reset(idc_handle h);
int idc_range_report(idc_handle h, int layer, idc_range_info* out);

/* ---- calibrated activation exponents (IDC_FP16X3) ------------------------------------------ *
 * act_exp[i] (integer, |a| <= 24) belongs to the output of layer i of the layer table (n_layers = what idc_num_layers answers for these
 * flags: the conv layers + 3; the non-conv rows are ignored): the tensor is stored as value * 2^a, so that a checkpoint whose activations
 * leave fp16's range (or sink below its normals) keeps all 22 bits of the two parts.  The scale costs nothing at run time: it is folded,
 * exactly (powers of two), into numbers the kernels read anyway -- the producer's BatchNorm scale / shift (layers without one: its bias and
 * accumulator scale; the ReLU is positively homogeneous), and the consumer's accumulator scale 2^-(wexp + a[input]).  NULL or all zeros gives
 * the blob of the plain call, byte for byte.  The packer resolves what the graph forces: a tensor has ONE exponent for all its consumers; the
 * fp32 island (conv1_1), fp32 outputs and conv10_2 (read by the head in its own epilogue) stay at 0; a shortcut conv takes the exponent of the
 * ConvTranspose it is summed into, and the two weight exponents of that pair are lowered until wexp + a[input] agree (one accumulator set, one
 * accumulator scale; the fused launch refuses to run on a blob where they differ).  The exponents in effect travel in the blob header
 * (header flag bit 0x100), idc_range_report returns them, and idc_get_activation returns UNSCALED values.
 * Non-zero exponents are refused with IDC_ERR_UNSUPPORTED for every other precision, and with IDC_FLAG_DIST_HEAD, IDC_FLAG_DIST313 or
 * IDC_FLAG_GLOBAL_HINTS (their heads / per-image shift read or add to tensors that would be scaled); n_layers that does not match is
 * IDC_ERR_INVALID_ARG. */
int idc_pack_weights_ex(int precision, unsigned flags, const idc_tensor_desc* tensors, int n_tensors, const int* act_exp, int n_layers,
                        void* blob, size_t blob_bytes);
int idc_load_weights_ex(idc_handle h, const idc_tensor_desc* tensors, int n_tensors, const int* act_exp, int n_layers);

/* ---- single operators (parity tests drive the same kernels the network uses) --------------- *
 * x NCHW fp32 [n,cin,h,w]; w/b in torch layouts; optional post-activation affine (eval-BN):
 * y = act(conv(x)+b [+ resid]) * bn_scale + bn_shift.  act: 0 none, 1 ReLU, 2 LeakyReLU(0.2).
 * in_stride=2 reads x[:, :, ::2, ::2] (model.py:149-151).  Output NCHW fp32.                  */
int idc_op_conv2d(int device_id, int precision, int n, int cin, int h, int w, const float* x,
                  int cout, int ksize, int dilation, int in_stride, const float* weight,
                  const float* bias, int act, const float* bn_scale, const float* bn_shift,
                  const float* resid, float* y);
/* ConvTranspose2d(k=4, s=2, p=1) (+ residual) (+act): weight (cin,cout,4,4); y [n,cout,2h,2w].  */
int idc_op_deconv4x4s2(int device_id, int precision, int n, int cin, int h, int w, const float* x,
                       int cout, const float* weight, const float* bias, int act,
                       const float* resid, float* y);
/* The fused pair of the decoder as ONE launch, planned as the network plans it (conv_ds_fused_m / _mh / _ms / _msh):
 * y = act(deconv4x4s2(x) + conv3x3(x_short) + b_deconv + b_short); x [n,cin,h,w], w_deconv (cin,cout,4,4), x_short [n,cin_short,2h,2w],
 * w_short (cout,cin_short,3,3) (dilation 1, padding 1); act 0 or 1; y [n,cout,2h,2w].  IDC_ERR_UNSUPPORTED where the network would run
 * the pair as two launches (grid below the large tile's threshold at the policy batch, cout not a multiple of 128, fp32). */
int idc_op_deconv_shortcut(int device_id, int precision, int n, int cin, int h, int w, const float* x, int cout,
                           const float* w_deconv, const float* b_deconv, int cin_short, const float* x_short,
                           const float* w_short, const float* b_short, int act, float* y);
/* The kernel the last single-operator call of this thread launched, as the layer table names it (idc_layer_info.kernel: template
 * arguments <WM,WP>, " splitK<n>"); a conv_ds_fused_m / _mh launch adds " half" (its 64-cout 4-wave form) or " 8-wave".  Empty when
 * the call failed before it chose a kernel.  The variant is chosen for idc_set_option("op_policy_batch", v) images (0 = the call's
 * own batch) while the launch carries the call's n. */
int idc_op_last_kernel(char* out, int cap);
/* Diagnostics of the capped grid-stride launches (test instrumentation, see option "grid_cap").  idc_grid_tag(i): the name of capped launch
 * site i = 0, 1, ..., NULL past the end.  idc_grid_last: what the last launch of site `tag` in this process asked for -- *want = the workgroups
 * that would cover all its items in one pass, *blocks = the grid it got = max(1, min(want, the launcher's cap, grid_cap)); want = 0 when the
 * site has not launched yet; an unknown tag: IDC_ERR_INVALID_ARG.  The record is process-wide, the last launch wins, and it is not
 * synchronised with other threads.  eval_sse records the x extent of its (x, image) grid. */
int idc_grid_last(const char* tag, long long* want, int* blocks);
const char* idc_grid_tag(int i);

#ifdef __cplusplus
}
#endif
#endif /* IDEEPCOLOR_H */
