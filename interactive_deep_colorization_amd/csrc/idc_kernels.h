// idc_kernels.h -- launch interface of the gfx950 kernels (internal; the public ABI is
// include/ideepcolor.h).
#pragma once
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "idc_grid.h"
#include "idc_resample.h"
#include "idc_layer.h"
#include "idc_ycc.h"
#include "idc_temporal.h"
#include "idc_motion.h"
#include "idc_track.h"

namespace idc {

// One implicit-GEMM convolution launch.  The output is computed over a grid of "sites":
// site (sy,sx) reads input pixels (sy*si + tap offsets) and writes output pixel
// (sy*so + ro[phase], sx*so + co[phase]).
//   conv3x3 (dilation d, reading x[::si, ::si]) : so=1, 1 phase, 9 taps, dy,dx in {-d,0,d}
//   ConvTranspose 4x4 s2 p1                     : si=1, so=2, 4 phases x 4 taps (2x2)
//   1x1 conv                                    : 1 tap, halo 0
struct ConvArgs {
    const void* in;         // NHWC [N][Hs*si][Ws*si][Cin]          (T)
    const void* wgt;        // packed [tap][kc][cout group][64][128B] (T), see idc_layout.h
    void* out;              // NHWC [N][Hs*so][Ws*so][CoutPad]       (T, or fp32 if out_f32)
    const void* resid;      // optional NHWC (fp32, or bf16 if resid_bf16), geometry of `out`: added before the activation
    const float* bias;      // [CoutPad]
    const float* bn_scale;  // optional [CoutPad]: y = act(.)*scale + shift  (eval-BN after ReLU)
    const float* bn_shift;
    const float* img_shift; // optional fp32 [N][CoutPad]: per-image vector added after the BN affine (global hints:
                            // glob_conv4norm_rep + conv4_3norm, models/global_model/deploy_nodist.prototxt:501-518)
    int N, Hs, Ws;
    int si, so;
    int nkc;                // Cin / KC   (KC = 128 B of channels)
    int ncg;                // CoutPad / 64
    int nphase, ntaps;
    int tiles_x, tiles_y;   // tiles per image
    int act;                // 0 none, 1 ReLU, 2 LeakyReLU(0.2)
    int out_f32;
    int resid_bf16;
    // split-K (conv_igemm only; small launches = the batch-1 click path): workgroup slice `sid` of ksplit
    // runs cin chunks [sid*kc_per, min(nkc, (sid+1)*kc_per)) and stores its raw fp32 accumulators to
    // partial[sid][output pixel][CoutPad]; splitk_epilogue then sums the slices in fixed order and applies
    // bias / shortcut / activation / BN.  ksplit <= 1: off.
    int ksplit, kc_per;
    float* partial;
    // fused input pack (conv_igemm, HALO = 0, the conv1_1 launch): when pk_L != nullptr the "halo" rows are not
    // loaded from `in` but built from the reference's input planes (NCHW fp32: L [N,1,H,W], ab [N,2,H,W],
    // mask [N,1,H,W]) -- model.py:139-148 (cast, mask - maskcent, cat(L/100, ab/110, mask)) fused with the im2col
    // of conv1_1: channel tap*4 + c of a site = normalised input c at 3x3 neighbour `tap`, zero outside the image
    // and for K >= 36.
    const float* pk_L;
    const float* pk_ab;
    const float* pk_mask;
    float pk_ldiv, pk_abdiv, pk_mmul, pk_mcent;
    // fused shortcut conv (conv_igemm_v2, deconv launches only): a 3x3 conv (pad 1, bias folded into
    // `bias`) of in2 = NHWC [N][2*Hs][2*Ws][nkc2 * 64] bf16 accumulated into the same output pixels;
    // wgt2 = its layout-2 weight image (same couts).  model.py:156,170,172.
    const void* in2;
    const void* wgt2;
    int nkc2;
    // fused regression head (conv_igemm_v2<2,*> only, when one workgroup owns all 128 couts):
    // head_out[n][c][y][x] = head_mul * tanh(head_b[c] + sum_k head_w[c][k] * y[k]), y = this layer's
    // fp32 result (not stored at all).  model_out + tanh + *110, model.py:108-109,174-175.
    const float* head_w;    // [2][128] or nullptr
    const float* head_b;    // [2]
    float* head_out;        // NCHW fp32 [N][2][Hs][Ws]
    float head_mul;
    // operand-split precisions (IDC_BF16X3 / IDC_BF16X6, conv_igemm_v2s / conv_igemm_v2ps in idc_v2m.hip): an fp32 value x travels as
    // `parts` bf16 values x = hi (+ mid) + lo; a pixel of a split tensor is [part][Cpad] bf16.  The K loop runs `nseg` segments of nkc
    // chunks each; segment s multiplies input part (seg_x >> 4s & 15) with weight part (seg_w >> 4s & 15) -- 3 segments (hi.hi, lo.hi,
    // hi.lo) or 6 (+ mid.hi, hi.mid, mid.mid), all into ONE fp32 accumulator set.  Weight part p starts w_part_bytes * p after a.wgt.
    // out_parts: parts written (0 with out_f32 / a fused head).  The shortcut sum (a.resid) is fp32 in these launches.
    int in_parts, out_parts, nseg;
    unsigned seg_x, seg_w;
    unsigned long long w_part_bytes;
    unsigned long long w_part_bytes2;   // ... of the fused shortcut conv's images (a.wgt2; conv_ds_fused_m's split form)
    const float* acc_scale; // IDC_FP16X3: one fp32 in device memory, 2^-s -- the layer's weight parts hold w * 2^s (a power of two: exact) so that the lo parts
                            // of small weights are NORMAL fp16 numbers (he-style weights ~0.02: lo ~1e-5 is subnormal, 6e-8 absolute = 2^-18 of the weight);
                            // the accumulators are multiplied by it when the bias joins.  nullptr = 1.0
    int split_f16;          // IDC_FP16X3: the parts are fp16 (11-bit) instead of bf16 (8-bit) values; same planes, same segments as IDC_BF16X3
    int warm;               // != 0: the throughput kernels pull their own code into L2 at entry (idc_warm_own_code below)
    const void* zeros;      // >= 16 zero bytes in device memory: LDS-DMA source of out-of-image halo rows (conv_click)
    int dy[36], dx[36], tw[36];   // [phase*9 + t]: tap offset in sites, packed-weight tap index
    int ro[4], co[4];
};

#ifdef __HIPCC__
// First-use cost of a kernel: on some boxes the first launch of a kernel after other kernels have run is
// 25-35 % (up to 36 us) slower on EVERY forward -- the launch fetches 17-37 KB of instructions it has not executed for ~1 GB of
// traffic, line after line (or page after page) as the wave reaches them.  One wave per workgroup therefore touches every 128-byte
// line of the kernel's own code at entry -- as DATA, by LDS-DMA into `lds_scratch` (256 bytes nobody reads; no destination register
// to keep alive) -- so that the lines are on their way into this XCD's L2, and their pages walked, all at once and under the prologue's
// own memory latency.  `lines` x 128 bytes from the current PC: callers pass LESS than their kernel's code size (codeLenInByte of the
// build, profiles/r04_kernel_resources.txt lists the kernels) unless other kernels follow it in the same code object.  The requests
// retire with the prologue's first vmcnt(0).
__device__ __forceinline__ void idc_warm_own_code(char* lds_scratch, int lane, int lines) {
    const char* const pc = (const char*)(__builtin_amdgcn_s_getpc() & ~(unsigned long long)127);
    for (int j = 0; j * 64 < lines; ++j)
        if (j * 64 + lane < lines)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(pc + (size_t)(j * 64 + lane) * 128),
                                             (__attribute__((address_space(3))) void*)lds_scratch, 4, 0, 0);
}
#endif

// Tuning / A-B knobs read from the environment exist only in the -DIDC_AB_PARTNERS build (make EXTRA=-DIDC_AB_PARTNERS: tools/ab_*.sh, tools/click_sweep.py,
// tools/probe_firstuse.sh); the default library reads ONE environment variable, IDC_RCCL_PATH (idc_rccl.hip), and is steered through idc_set_option only.
#ifdef IDC_AB_PARTNERS
static inline int idc_env_int(const char* name, int dflt) { const char* v = getenv(name); return (v && *v) ? atoi(v) : dflt; }
#else
static inline int idc_env_int(const char*, int dflt) { return dflt; }
#endif

struct ConvConfig { int wm, wp; };     // waves along cout (x64) and along pixel rows (x4 rows of 16)

// precision: 0 fp32, 1 bf16.  halo: 0,1,2.  Returns hipSuccess or the launch error.
hipError_t launch_conv(int precision, ConvConfig cfg, int halo, const ConvArgs& a, hipStream_t s);
// conv_igemm's and conv_click's 32-bit source offsets: one source image of at most 2^31 bytes (hipErrorInvalidConfiguration from both launchers otherwise;
// plan_forward refuses such a layer with the reason).  No family of the default library goes further for these launches, so this is the engine's limit.
bool conv_igemm_offsets_fit(int Hs, int Ws, int si, int nkc);
// Large-tile bf16 throughput kernel (32x32x16 MFMA, 8 waves, LDS-DMA weights).  cfg = {WCO, WPX}:
// {4,2} = 256 couts x (32x8 sites), {2,4} = 128 couts x (32x16 sites).  a.wgt must point at the
// layer's layout-2 weight image (idc_layout.h); tiles_x/tiles_y count 32 x 4*WPX tiles.
hipError_t launch_conv_v2(ConvConfig cfg, int halo, const ConvArgs& a, hipStream_t s);
// The same tile from v_mfma_f32_16x16x32_bf16 (idc_v2m.hip: the more energy-efficient MFMA shape on a power-capped chip).  a.wgt must
// point at the layer's LAYOUT-1 image; bf16-output launches without shortcut sum / per-image shift only (conv_v2m_applies), else
// hipErrorInvalidConfiguration.
hipError_t launch_conv_v2m(ConvConfig cfg, int halo, const ConvArgs& a, hipStream_t s);
bool conv_v2m_applies(const ConvArgs& a);
// ... and its 3x3 form without address arithmetic in the K loop (conv_igemm_v2p: padded halo rows, unrolled taps, buffer loads)
hipError_t launch_conv_v2p(ConvConfig cfg, int halo, const ConvArgs& a, hipStream_t s);
bool conv_v2p_applies(ConvConfig cfg, int halo, const ConvArgs& a);
hipError_t init_kernels_v2m();
// Operand-split form of the same tiles (conv_igemm_v2s: every geometry conv_igemm_v2m covers; conv_igemm_v2ps: the 3x3 forms of
// conv_igemm_v2p): a.in / a.out are split tensors (in_parts / out_parts), a.wgt the layout-1 images of the weight parts, shortcut sum
// fp32, fp32 output / per-image shift / LeakyReLU / fused head supported.  hipErrorInvalidConfiguration if the launch does not qualify.
hipError_t launch_conv_v2s(ConvConfig cfg, int halo, const ConvArgs& a, hipStream_t s);
hipError_t launch_conv_v2ps(ConvConfig cfg, int halo, const ConvArgs& a, hipStream_t s);
bool conv_v2s_applies(const ConvArgs& a);
bool conv_v2ps_applies(ConvConfig cfg, int halo, const ConvArgs& a);

// ConvTranspose 4x4 s2 + the 3x3 shortcut conv it is summed with, one K loop (conv_ds_fused); a.in2 / wgt2 / nkc2 = the
// shortcut's input, layout-2 weights and channel chunks, a.bias = the two biases added.  hipErrorInvalidConfiguration if
// the launch does not qualify.
hipError_t launch_conv_ds(const ConvArgs& a, hipStream_t s);
// The same launch from v_mfma_f32_16x16x32_bf16 (idc_dsm.hip: conv_ds_fused_m); a.wgt / a.wgt2 = the LAYOUT-1 images
hipError_t launch_conv_ds_m(const ConvArgs& a, hipStream_t s);
// ... and its operand-split form (conv_ds_fused_ms / _msh: split tensors in and out, fp32 accumulation of both K loops, split epilogue)
hipError_t launch_conv_ds_ms(const ConvArgs& a, hipStream_t s);
bool conv_ds_m_fits(int Hs, int Ws, int nkc, int nkc2);   // (else conv_ds_fused, which addresses with 64-bit pointers)
bool conv_ds_m_applies(const ConvArgs& a);
bool conv_ds_m_half(const ConvArgs& a);   // launch_conv_ds_m runs its 64-cout, 4-wave form for this launch
bool conv_ds_ms_applies(const ConvArgs& a);
hipError_t init_kernels_dsm();
void set_ds_half(int v);              // 1 (default): grids with fewer 128-cout workgroups than CUs run the 64-cout, 4-wave form of conv_ds_fused_m
// model1 = conv1_1 + conv1_2 of a 32x32 tile in one workgroup (conv1_block_fused): `a` = conv1_1's arguments with conv1_2's
// riding in (wgt2 = its layout-1 weights, head_b = its bias, bn_scale/bn_shift, out = its output)
hipError_t launch_conv1_block(const ConvArgs& a, hipStream_t s);
bool conv1_block_applies(const ConvArgs& a);
// conv1_1 as the exact-fp32 island of an operand-split handle (conv1_1_split_kernel: fp32 MFMA straight from the input patch, a.out_parts planes out)
hipError_t launch_conv1_1_split(const ConvArgs& a, hipStream_t s);
bool conv1_1_split_applies(const ConvArgs& a);
// conv1_2 of an operand-split handle on conv1_block_fused_t's conv1_2 tile (conv1_2_split_kernel: 32 x 12 pixels, two workgroups per CU, segments over a static halo)
hipError_t launch_conv1_2_split(const ConvArgs& a, hipStream_t s);
bool conv1_2_split_applies(const ConvArgs& a);
// conv1_1 (4 -> 64, input pack fused) as one 32x32 tile per workgroup, bf16 (-DIDC_AB_PARTNERS build only: the default library's predicate is false)
hipError_t launch_conv1_1_bf16(const ConvArgs& a, hipStream_t s);
bool conv1_1_bf16_applies(const ConvArgs& a);
// Batch-1 click-path kernel (conv_click): tile 16 x 4*wp sites x 64 couts, the workgroup's whole K slice (kc_per chunks x
// all taps) requested by LDS-DMA at entry; a.kc_per <= conv_click_max_chunks(wp, halo, ntaps), a.ksplit = ceil(nkc / kc_per),
// a.tiles_x / tiles_y count 16 x 4*wp tiles, a.zeros set.  Layout-1 weights.
hipError_t launch_conv_click(int precision, int wp, int halo, const ConvArgs& a, hipStream_t s);
int conv_click_max_chunks(int wp, int halo, int ntaps);
// Second half of a split-K launch: out = act(sum_s partial[s] + bias [+ resid]) [* bn_scale + bn_shift] [+ img_shift]
// over all N*Hout*Wout*CoutPad outputs (geometry and epilogue fields taken from the same ConvArgs).
hipError_t launch_splitk_epilogue(int precision, const ConvArgs& a, hipStream_t s);
// fp32 Winograd F(2x2,3x3) form of a 3x3 stride-1 conv (idc_wino.hip): a.wgt = the layer's U image, a.out fp32,
// a.dy[8] = dilation (1 | 2); hipErrorInvalidConfiguration if the launch does not qualify
hipError_t launch_conv_wino(int precision, const ConvArgs& a, hipStream_t s);     // precision 1: conv_wino_bf16 (batch-1 click path only)
// fp32 ConvTranspose 4x4 s2 as Winograd F(2x2,2x2) over its four phases: a.wgt = the 36-position U image, a.Hs / a.Ws = input size
hipError_t launch_deconv_wino(int precision, const ConvArgs& a, hipStream_t s);    // precision 1: the bf16 twin (click path)
// the launch guards of the two entry points above as a predicate (args filled in: in / wgt / zeros / resid / out_f32 set), and the
// 32-bit source-offset bound alone (known before the pointers are: set_geometry)
bool conv_wino_applies(int precision, const ConvArgs& a, bool deconv);
// bf16 click path (idc_kw.hip): a 3x3 stride-1 conv with K split over the waves of a workgroup, no reduction launch; a.wgt = the
// layer's LAYOUT-1 image, a.dy[8] = dilation, a.zeros set; hipErrorInvalidConfiguration if the launch does not qualify
hipError_t launch_conv_kwave(const ConvArgs& a, hipStream_t s);
bool conv_kwave_applies(const ConvArgs& a);
hipError_t init_kernels_kw();
// conv_kwave_chain_bf16 (idc_kw.hip, round 5): a run of consecutive same-shape 8-chunk conv_kwave_bf16 layers (the 512 -> 512 trunk of
// the bf16 click path: conv4_2 .. conv7_3 at batch 1) as ONE persistent launch, a grid barrier between layers instead of a launch floor.
struct KwChainLayer {
    const void* in; void* out; const void* wgt; const float* bias; const float* bn_scale; const float* bn_shift;
    int act;                // 0 none, 1 ReLU, 2 LeakyReLU(0.2)
    int d;                  // dilation 1 | 2
};
constexpr int kKwChainMax = 12;
struct KwChainArgs {
    int nlayers, H, W, N, ncg;
    unsigned spin_limit;            // polls of the barrier counters before a workgroup gives up (sets *abort_flag, leaves)
    unsigned long long* bar;        // eight device counters 128 bytes apart (one per blockIdx & 7), monotone: + its arrivals per barrier
    unsigned long long bar_base;    // barriers done by every earlier launch of the handle (counter c then holds bar_base x arrivals_of(c))
    int* abort_flag;                // host-visible (pinned) int: set to 1 by a workgroup that gave up
    long long* stamps;              // diagnostic (IDC_KW_STAMPS=1), else null: [workgroup][layer][8] cycle stamps of the phases of a layer
    KwChainLayer layer[kKwChainMax];
};
// workgroups of one layer (the same for every layer of a chain: 8x8-pixel tiles x parities x images x 32-cout groups), 0 if the shape is not covered
int conv_kwave_chain_blocks(int H, int W, int N, int ncg, int d);
// workgroups of the chain kernel the device holds at once (one per CU: 104 KiB of LDS each); 0 on error
int conv_kwave_chain_capacity(int device);
// mode 1: hipLaunchCooperativeKernel (the runtime guarantees co-residency or fails cleanly); mode 2: plain launch (caller checked the capacity)
hipError_t launch_conv_kwave_chain(const KwChainArgs& c, int blocks, int mode, hipStream_t s);
bool wino_offsets_fit(int Hs, int Ws, int si, int nkc);
hipError_t init_kernels_wino();
void set_wino_form(int form);      // 0 = by grid size, 12 / 21 / 22 = force conv_wino_f32<TB,CB> (speed only)
// One-time: raise the dynamic-LDS limit of every conv instantiation.
hipError_t init_kernels();
size_t conv_lds_bytes(ConvConfig cfg, int halo);

// conv1x1(128->2) + tanh + *out_mul, NHWC (T) -> NCHW fp32
hipError_t launch_head(int precision, const void* x, const float* w, const float* b, float* out,
                       int N, int H, int W, float out_mul, hipStream_t s);
// softmax over the first `nclass` of `cstride` fp32 logits per pixel, * temperature first;
// NHWC fp32 logits [npix][cstride] -> NCHW fp32 probabilities [N][nclass][H][W]
hipError_t launch_softmax_nchw(const float* logits, float* out, int N, int H, int W, int nclass,
                               int cstride, float temperature, hipStream_t s);
// 313-bin head tail (models/reference_model/deploy_nopred.prototxt:776-850): logits fp32 NHWC [N][H/4][W/4][cstride]
// (313 valid) -> the two grouped bilinear x2 deconvs (fixed kernel, colorize_image.py:410-413; per axis
// out[4m+j] = ((4-j) in[m] + j in[m+1]) / 4 with in[M] = 0) -> per full-resolution pixel
//   dist_S [N][313][H][W] = softmax(S * l)  (optional, may be nullptr)
//   pred_ab [N][2][H][W]  = sum_q softmax(2.6 * l)_q * w_ab[c][q] + b_ab[c]
// w_ab: fp32 [2][313] then [2] bias.
hipError_t launch_dist313(const float* logits, const float* w_ab, float* pred_ab, float* dist_S, int N, int H, int W,
                          int cstride, float S, float T, hipStream_t s);

// Global-hints branch (models/global_model/deploy_nodist.prototxt:37-172): per image
//   y1 = BN1(relu(Wg g + bg + Ws s + bs)),  y_{i+1} = BN_{i+1}(relu(W_{i+1} y_i + b_{i+1})), i = 1..3  ->  out [N][512]
// in [N][316] = 314 histogram+flag values then the 2 saturation values; params = the packed fp32 section
// described at glob_param_floats() (transposed weights [k][512], then bias / BN scale / BN shift).
hipError_t launch_glob_branch(const float* in, const float* params, float* out, int N, hipStream_t s);
constexpr int kGlobIn = 316, kGlobC = 512;
constexpr size_t glob_param_floats() { return (size_t)kGlobIn * kGlobC + 3 * kGlobC + 3 * ((size_t)kGlobC * kGlobC + 3 * kGlobC); }

// Lab -> sRGB uint8 (+ optional rgb -> Lab refresh), float64 like skimage (colorize_image.py:20-28,31-36):
// L [N,1,H,W] fp32 (+ l_add), ab [N,2,H,W] fp32 -> rgb [N,H,W,3] u8, lab_q [N,3,H,W] f64 (or nullptr)
hipError_t launch_pcie_copy(void* dst, const void* src, size_t bytes, hipStream_t s);   // small host <-> device copies as a kernel on the forward's stream
hipError_t launch_lab_post(const float* L, float l_add, const float* ab, unsigned char* rgb, double* lab_q, int N,
                           int H, int W, hipStream_t s);

// Display / full-resolution step (ui/gui_draw.py:280-283, colorize_image.py:123-158): (a, b) planes [H,W] (fp32 or fp64)
// resized to [oh,ow] -- interp 0 cv2 INTER_CUBIC, 1 scipy zoom order 1, 2 scipy zoom order 0 -- then Lab -> sRGB uint8
// with L_out [oh,ow] (float64) -> rgb [oh,ow,3]
hipError_t launch_upsample_lab2rgb(const void* a_plane, const void* b_plane, int src_f64, int H, int W, int interp, const double* L_out,
                                   int oh, int ow, unsigned char* rgb, hipStream_t s);

// Colour picker (data/lab_gamut.py).  gamut_map: abGrid(gamut_size, D).update_gamut(L[k]) for k < n -- grid side A, point (i, j) = (a, b) =
// (-gamut_size + i D, -gamut_size + j D) -> pts [n,A,A,3] u8 (truncated), mask [n,A,A] u8 (1: the uint8 colour is within 1.0 of the point in
// Lab), masked [n,A,A,3] u8 = mask ? pts : 255; each output may be nullptr.  snap_colors: snap_ab(L[k], rgb[k]) for k < n -> rgb_out [n,3] u8,
// lab_out [n,3] f64 = rgb2lab(rgb_out), iters [n] = loop iterations run (1..20); each may be nullptr.  float64, nothing but their arguments is touched.
hipError_t launch_gamut_map(const double* L, int n, int gamut_size, int D, int A, unsigned char* pts, unsigned char* masked, unsigned char* mask,
                            hipStream_t s);
hipError_t launch_snap_colors(const double* L, const unsigned char* rgb, int n, unsigned char* rgb_out, double* lab_out, int* iters, hipStream_t s);

// Global statistics (global_stats.prototxt): rgb u8 [N,H,W,3] -> counts [N][313] (uint32, zeroed by the caller) of
// the 4x4-pooled ab values' nearest centre, and sat_sum [N] (float64, zeroed) = sum of HSV saturation over pixels.
hipError_t launch_global_stats(const unsigned char* rgb, const float* centres, unsigned* counts, double* sat_sum, int N,
                               int H, int W, hipStream_t s);

// Reference-image global hints (idc_global_stats_rgb / idc_set_global_refs / idc_forward_async_rgb_ref; idc_colour.hip).
// ref_stats: launch_global_stats for m references of INDIVIDUAL sizes, each sampled to the net size [H,W] by launch_ingest's rule inside the
// kernel: refs [m] = {byte offset into packed, h, w}, packed = the [h,w,3] u8 images back to back (no alignment asked) -> counts [m][313]
// (uint32, zeroed by the caller) and sat_part [m][ref_stats_workgroups(H, W)] (float64, every entry written): the saturation sum of each of
// a reference's workgroups, reduced in a fixed order.  A reference's figures depend on nothing but its own pixels and (H, W).
// glob_rows: row i < n of rows [n][kGlobIn], the layout launch_glob_branch reads, from reference r = ref_index[i] (< 0: 316 zeros):
// counts[r] / nblk, hist_flag, and with_sat ? {sum of sat_part[r] in index order / (H*W), 1} : {0, 0}; and, where hist != nullptr, hist
// [m][313] and s_avg [m] (or nullptr) of every reference, idc_global_histogram's expressions.  n or m may be 0.
struct RefDesc { long long off; int h, w; };
int ref_stats_workgroups(int H, int W);
hipError_t launch_ref_stats(const RefDesc* refs, int m, const unsigned char* packed, const float* centres, int H, int W, unsigned* counts,
                            double* sat_part, hipStream_t s);
hipError_t launch_glob_rows(const unsigned* counts, const double* sat_part, const int* ref_index, int n, int m, int H, int W, float hist_flag,
                            int with_sat, float* rows, float* hist, float* s_avg, hipStream_t s);

// Click session (idc_session.hip).  HintRect = idc_hint of include/ideepcolor.h after clipping: inclusive rectangle,
// (c0,c1) = ab (mode 0) or (c0,c1,c2) = RGB 0..255 (mode 1).  raster_hints fills ab [2,H,W] and mask [1,H,W] of ONE
// image: the last covering hint wins; uncovered pixels get ab = 0, mask = 0 (a black canvas is Lab (0,0,0)).
struct HintRect { int y0, x0, y1, x1; float c0, c1, c2; };
hipError_t launch_raster_hints(const HintRect* hints, int n_hints, int mode, float mask_value, float* ab, float* mask,
                               int H, int W, hipStream_t s);

// Image kernels (idc_colour.hip): a source image on the device to the net's input, and the net's result back to the source's size.  Five
// launchers, each ONE kernel template over the source format.  bits = 0: [h,w,3] u8 RGB; 8 | 16: one plane [h,w] of u8 | u16 samples whose value
// stands on all three channels (idc_set_image_gray; the rule: include/ideepcolor.h).  out_bits = 8 | 16: the image goes out as u8 | u16 [.,.,3]
// (16 only from 16-bit samples).  Grids: RGB launches walk a capped grid (idc_grid.h) in a grid-stride loop; grey launches are exact.
//
// ImgDesc: images of INDIVIDUAL sizes packed back to back (idc_forward_async_images / _gray).  imgs [n+1]: entry i = {byte offset of image i in
// src, pixels of images 0..i-1, h, w}; no alignment is asked of an image's start, and entry n = {all bytes, all pixels, 0, 0} closes the run.
// imgs == nullptr where a launcher allows it: a uniform run of n images of sh x sw (RGB only; for launch_joint_fullres also ONE plane, n = 1).
struct ImgDesc { long long off, first; int h, w; };

// Ingestion (colorize_image.py:52-77): srcs [n] device pointers to [src_h,src_w,C] images -> bilinear net-size net [n,H,W,C] of the sample type
// (colorspace.resize_bilinear_u8's rule, float64; the identity at src == net size), lab_net [n,C,H,W] f64 = rgb2lab of it -- (L, a, b) of an
// RGB image, L of a plane -- (either may be nullptr) and Lp [n][H*W] fp32 = L - l_cent, in one launch.
hipError_t launch_ingest(int bits, const void* const* srcs, int n, int src_h, int src_w, int H, int W, float l_cent, float* Lp, void* net,
                         double* lab_net, hipStream_t s);

// Full-resolution getters (colorize_image.py:123-158) from the resident source src [oh,ow,C]: L = rgb2lab(src)[0] (mask == nullptr) or
// 50 * zoom(mask, order 0) / mask_value (mask [H,W] fp32; mask_value 0: L = 0), (a, b) planes [H,W] (fp32 or fp64; nullptr: a = b = 0)
// resized as in launch_upsample_lab2rgb, Lab -> sRGB -> rgb [oh,ow,3].  src and rgb 4-byte aligned.
hipError_t launch_fullres(int bits, const void* src, int oh, int ow, const void* a_plane, const void* b_plane, int src_f64, int H, int W, int interp,
                          const float* mask, float mask_value, void* rgb, int out_bits, hipStream_t s);

// Pipelined batches, ONE launch each for all n images.
// prologue: the packed sources -> Lp [n][H*W] = L - l_cent by launch_ingest's rule from image i's own size and start, and per pixel the LAST
// hint of hints[offs[i] .. offs[i+1]) (already clipped, as for launch_raster_hints) that covers it -> ab [n,2,H,W], mask [n,1,H,W];
// offs == nullptr: no image has hints.
// packed_fullres: launch_fullres's pixel (L of the source pixel, (a, b) = planes 1 and 2 of image i's lab_q [n,3,H,W] f64 resized by `interp`)
// for every pixel of the run -> rgb, packed as src is (image i at element 3 * first); src and rgb 4-byte aligned at their base only.
// total = imgs[n].first, the pixels of the run (read only with a table; a uniform run has n * oh * ow).
hipError_t launch_prologue(int bits, const void* src, const ImgDesc* imgs, int n, int sh, int sw, int H, int W, float l_cent, const int* offs,
                           const HintRect* hints, int mode, float mask_value, float* Lp, float* ab, float* mask, hipStream_t s);
hipError_t launch_packed_fullres(int bits, const void* src, const ImgDesc* imgs, int n, int oh, int ow, long long total, const double* lab_q, int H,
                                 int W, int interp, void* rgb, int out_bits, hipStream_t s);

// Joint bilateral ab upsampling (idc_fullres_rgb with IDC_INTERP_JOINT, idc_fullres_ab, the source-size epilogue of the pipelined calls while
// idc_set_batch_upsample is JOINT; the rule: include/ideepcolor.h).  One workgroup per 32 x 8 output tile on an exact grid
// dim3(max_tiles, n): max_tiles = joint_tiles of the largest image.  Image i reads the planes a_plane / b_plane + i * plane_stride elements
// ([H,W] fp32 or fp64; both nullptr: a = b = 0) and, for interp 3, the guide Lp + i * H * W (fp32, L - l_cent) with
// jp = {R, 2 sigma_s^2, 2 sigma_r^2}; interp 0..2: launch_fullres's rules.
// -> rgb (packed as src is, any alignment, u16: even; or nullptr) and ab_out (or nullptr): image i's [2,h,w] f64 at 2 * first_i.
struct JointParams { int R; double two_ss, two_sr; };
inline long long joint_tiles(int h, int w) { return (long long)((h + 7) / 8) * ((w + 31) / 32); }
hipError_t launch_joint_fullres(int bits, const void* src, const ImgDesc* imgs, int n, int sh, int sw, long long max_tiles, const void* a_plane,
                                const void* b_plane, int src_f64, long long plane_stride, const float* Lp, float l_cent, int H, int W, int interp,
                                JointParams jp, void* rgb, int out_bits, double* ab_out, hipStream_t s);

// Antialiased ingestion (idc_set_ingest_filter; idc_resample.hip; the rule: include/ideepcolor.h): the pre-pass that writes the net-size lattice
// image [H,W,channels] of each of the njobs down-scaled images (ResampleJob, idc_resample.h: byte offsets from src_base / dst_base, the image's
// own tiling) -- uint8 x 3, uint8 x 1 or uint16 x 1.  Exact grid dim3(max_tiles, H, njobs), max_tiles = the largest jobs[.].tiles.
hipError_t launch_resample(const void* src_base, void* dst_base, const ResampleJob* jobs, int njobs, int max_tiles, int bits, int channels, int H,
                           int W, hipStream_t s);

// Painted hint layers (idc_set_hints_layer / idc_forward_async_layers; idc_layer.hip; the rule: include/ideepcolor.h): the post-pass behind the
// prologue or raster_hints.  layers = the [h,w,4] u8 RGBA layers packed back to back from a 16-byte aligned base, descs [n] (LayerDesc,
// idc_layer.h: h == 0 = no layer); ab [n,2,H,W] and mask [n,1,H,W] are composed in place; cells [n] += the cells each layer hinted (the caller
// zeroes it on the same stream).  Exact grid dim3(max_blocks, n), max_blocks = the largest layer_blocks among the layers.
hipError_t launch_hint_layers(const unsigned char* layers, const LayerDesc* descs, int n, int max_blocks, int H, int W, int alpha_min, int cover,
                              float mask_value, float* ab, float* mask, int* cells, hipStream_t s);

// YCbCr 4:2:0 output planes (idc_set_batch_output / idc_fullres_ycc / idc_rgb_to_ycc420; idc_ycc.hip; the rule: include/ideepcolor.h): the
// post-pass behind the epilogues.  rgb = the packed [h,w,3] u8 results from a 4-byte aligned base, descs [n] (YccDesc, idc_ycc.h: where image
// i's RGB starts in rgb and its plane block in out, and its size); out = the packed blocks from a 4-byte aligned base; format IDC_OUT_I420 |
// IDC_OUT_NV12, matrix IDC_YCC_*.  Exact grid dim3(max_blocks, n), max_blocks = the largest ycc_blocks among the images.
hipError_t launch_ycc420(const unsigned char* rgb, const YccDesc* descs, int n, int max_blocks, int format, int matrix, unsigned char* out,
                         hipStream_t s);

// Motion-adaptive temporal ab filter (idc_set_temporal_filter / idc_temporal_apply; idc_temporal.hip; the rule: include/ideepcolor.h; the
// geometry: idc_temporal.h).  L [n,H,W] fp32 = the frames' L planes, l_prev [H,W] / y_prev [2,H,W] the sequence state (read only with have != 0),
// x [n,2,H,W] fp32 the network's ab maps, overwritten by y; g float64 [n,H,W] and part float64 [n, temporal_partials] the scratch the first
// launch fills for the second; D float64 [n] and cut_flags int32 [n] what the call reports.  Every pointer but part, D and cut_flags is 16-byte
// aligned.  Exact grids: dim3(temporal_tiles, n) and temporal_blend_blocks; cut = 0 never cuts.
hipError_t launch_temporal_diff(const float* L, const float* l_prev, int have, int n, int H, int W, int radius, double strength, double sigma,
                                double* g, double* part, hipStream_t s);
hipError_t launch_temporal_blend(float* x, const double* g, const double* part, const float* L, float* y_prev, float* l_prev, int have, int n,
                                 int H, int W, double cut, double* D, int* cut_flags, hipStream_t s);

// Block-matched motion compensation of that filter (idc_set_temporal_motion; idc_motion.hip; the geometry: idc_motion.h).  v int8 [n, H/8, W/8, 2]
// (dy, dx): written by the search for all n frames, read by the other two.  launch_motion_diff: launch_temporal_diff on the warped predecessor.
// launch_motion_blend: ONE frame -- x [2,H,W] becomes y, y_before [2,H,W] is the previous frame's filtered map in ANOTHER buffer (never written
// here: the caller copies the state behind the last frame), g / part / v / D / cut_flag this frame's; pass = no predecessor.  Exact grids.
hipError_t launch_motion_search(const float* L, const float* l_prev, int have, int n, int H, int W, int search, double penalty, int8_t* v,
                                hipStream_t s);
hipError_t launch_motion_diff(const float* L, const float* l_prev, const int8_t* v, int have, int n, int H, int W, int radius, double strength,
                              double sigma, double* g, double* part, hipStream_t s);
hipError_t launch_motion_blend(float* x, const float* y_before, const double* g, const double* part, const int8_t* v, int pass, int H, int W,
                               double cut, double* D, int* cut_flag, hipStream_t s);

// Hints that follow those vectors (idc_set_hint_tracking; idc_track.hip; the walk and the sizes: idc_track.h).  ONE launch for all n frames: the
// RAW own planes ab [n,2,H,W] / mask [n,H,W], L [n,H,W], l_prev, v of launch_motion_search on the same L, and the state (A [2,H,W], M, G [H,W]) are
// read; the tracked planes go to out_* -- other buffers: the walks read the raw planes of earlier frames.  have_prev: frame 0 has a predecessor
// (the search's `have`); have_state: the state holds a frame.  The caller copies the last frame to the state BEHIND the launch.  Exact grid.
hipError_t launch_track_hints(const float* ab, const float* mask, const float* L, const float* l_prev, const int8_t* v, const float* state_ab,
                              const float* state_mask, const int32_t* state_age, int have_prev, int have_state, int n, int H, int W, int life,
                              double tol, float* out_ab, float* out_mask, int32_t* out_age, hipStream_t s);

// Evaluation batches (idc_reveal_hints / idc_forward_async_eval; idc_colour.hip).  reveal_hints: (c0, c1) of each of the n_rects clipped
// rectangles of `hints` = the float64 mean ab (rounded once to fp32) of its image's net-size pixels under it, one workgroup per rectangle, fixed
// summation order, cost = the rectangle's area; the image is the single [src_h,src_w,3] source at src (imgs == nullptr) or image i of the packed
// run with offs[i] <= k < offs[i+1] (offs [n+1]: the list's offsets).  colours (or nullptr) [.,2] gets the same pair at index orig[k].
// ragged_net_truth: rgb_net [n,H,W,3] = every image resized to the net size (the prologue's uint8 pixel).  eval_sse: sse [n][3] += the sum of
// squared differences of res and truth per image and channel (R, G, B), both packed alike from 4-byte aligned bases: n images of hw pixels
// (imgs == nullptr) or the ImgDesc run; max_pixels / total_pixels = the largest image / all images.  The caller zeroes sse on the same stream.
hipError_t launch_reveal_hints(const unsigned char* src, const ImgDesc* imgs, const int* offs, int n, int src_h, int src_w, int H, int W,
                               HintRect* hints, int n_rects, const int* orig, float* colours, hipStream_t s);
hipError_t launch_ragged_net_truth(const unsigned char* src, const ImgDesc* imgs, int n, int H, int W, unsigned char* rgb_net, hipStream_t s);
hipError_t launch_eval_sse(const unsigned char* res, const unsigned char* truth, const ImgDesc* imgs, int n, long long hw, long long max_pixels,
                           long long total_pixels, unsigned long long* sse, hipStream_t s);
// Distribution scores, the ground truth (idc_colour.hip, beside the reveal kernel whose device functions and summation order it shares): truth
// [n][2][(H/s)*(W/s)] fp32 = reveal_hints' colour of every cell's s x s rectangle (s = 1 or 4), bit for bit; image i of the packed run imgs, or
// (imgs == nullptr, n == 1) the single [src_h,src_w,3] source at src.
hipError_t launch_dist_truth(const unsigned char* src, const ImgDesc* imgs, int n, int src_h, int src_w, int H, int W, int s, float* truth,
                             hipStream_t st);

// Colour suggestions at one pixel (get_ab_reccs, colorize_image.py:322-354): see idc_session.hip for the algorithm.
// pdf bin b at pdf[b*stride]; centres [B][2]; out_centres [K][2], out_conf [K] (f64); out_counts [B] or nullptr.
constexpr int kSuggestMaxBins = 1024, kSuggestMaxK = 16;
hipError_t launch_suggest(const float* pdf, long long stride, int B, const float* centres, int K, int N, unsigned seed,
                          double* out_centres, double* out_conf, unsigned* out_counts, hipStream_t s);
// The same body for nq queries in one launch (workgroup = query): dist [n][B][Hd][Wd], s = 4 (529 head) or 1 (313 head); queries [nq], or
// peaks != nullptr: query q = peak q of dist_peaks' [n][P][2] buffer, image q / P, seed seed0 + q.  out_centres [nq][K][2], out_conf [nq][K]; the
// empty query (-1, -1) and anything outside the batch or the image write zeros.
struct DistQuery { int img, y, x; unsigned seed; };
hipError_t launch_suggest_batch(const float* dist, int n, int B, int Hd, int Wd, int s, const DistQuery* queries, const int* peaks, int P,
                                unsigned seed0, int nq, const float* centres, int K, int N, double* out_centres, double* out_conf,
                                hipStream_t st);

// Maps of the resident distribution dist [n][B][npix] (idc_session.hip): ent [n][npix] = sum_q p log p (fp64 sum, p == 0 -> 0);
// decode -> ab [n][2][npix] and conf [n][npix] = p_max (or nullptr): mode 0 the arg-max bin's centre (ties -> lowest bin), mode 1
// the mean of centres [B][2] under weights (p / p_max)^gamma.  The result of an image does not depend on n.
hipError_t launch_dist_entropy(const float* dist, int n, int B, int npix, float* ent, hipStream_t s);
hipError_t launch_dist_decode(const float* dist, int n, int B, int npix, int mode, float gamma, const float* centres, float* ab,
                              float* conf, hipStream_t s);
// Uncertainty peaks of the entropy map ent [n][Hd][Wd] (launch_dist_entropy's): P rounds of "smallest ent, ties -> lowest cell index, then every
// cell with max(|dy|, |dx|) < radius leaves" per image, cells under a non-zero s x s block of mask [n][Hd*s][Wd*s] (or nullptr) left out;
// peaks [n][P][2] = (cy*s + s/2, cx*s + s/2) or (-1, -1), peak_ent [n][P] (or nullptr); work [n][Hd*Wd] floats of scratch.
hipError_t launch_dist_peaks(const float* ent, const float* mask, int n, int Hd, int Wd, int s, int P, int radius, float* work, int* peaks,
                             float* peak_ent, hipStream_t st);
// Distribution scores (include/ideepcolor.h, idc_dist_score: definitions 2-7) of dist [n][B][npix] against truth [n][2][npix] (launch_dist_truth):
// the nn nearest of centres [B][2] per cell, cross-entropy against their soft encoding, rank of the nearest bin.  part [n][ceil(npix/64)] doubles of
// scratch: the block sums; xent [n] = their fixed-order fold (a second, one-wave-per-image launch); hits [n][ranks.n] (or nullptr with ranks.n
// == 0; zeroed here on the same stream); xent_map / rank_map / target [n][npix] may each be nullptr.  B <= kSuggestMaxBins, nn in 1..min(16, B).
struct ScoreRanks { int n; int thr[8]; };
hipError_t launch_dist_score(const float* dist, const float* truth, const float* centres, int n, int B, int npix, int nn, float sigma,
                             ScoreRanks ranks, double* part, double* xent, unsigned* hits, double* xent_map, int* rank_map, int* target,
                             hipStream_t st);

// Range audit (idc_audit.hip; idc_set_range_audit): one layer's sticky record in device memory, and the streaming reduction that folds a stored
// tensor into it -- npix pixels of [parts][Cpad] 16-bit values (bf16, or fp16 when f16; value = sum of the parts) or, parts = 0, of [Cpad] fp32;
// channels >= C are padding and skipped.  max_abs over the finite values (atomicMax on the bit pattern); |value| >= 65504 counts as saturated in
// the fp16 forms only; non-zero |value| < 2^-14 counts as tiny in every form.
struct AuditRecord {
    unsigned max_abs_bits, pad;
    unsigned long long n_saturated, n_tiny, n_nonfinite;
};
hipError_t launch_range_audit(const void* src, long long npix, int C, int Cpad, int parts, int f16, AuditRecord* rec, hipStream_t s);

// layout converters for the single-operator test entry points and idc_get_activation
hipError_t launch_nchw_to_nhwc(int precision, const float* src, void* dst, int N, int C, int H, int W,
                               int Cpad, hipStream_t s);
hipError_t launch_nhwc_to_nchw(int src_is_bf16, const void* src, float* dst, int N, int C, int H,
                               int W, int Cstride, hipStream_t s);
// ... of a split tensor: dst = sum over the `parts` bf16 planes of a pixel (fp32 sum, hi first)
hipError_t launch_split_to_nchw(const void* src, float* dst, int N, int C, int H, int W, int Cpad, int parts, int f16, hipStream_t s);
// fp32 NCHW -> split NHWC (single-operator test entry points)
hipError_t launch_nchw_to_split(const float* src, void* dst, int N, int C, int H, int W, int Cpad, int parts, int f16, hipStream_t s);

}  // namespace idc
