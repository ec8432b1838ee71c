// idc_engine.h -- what the host units of libideepcolor_hip.so share (idc_pack / idc_plan / idc_exec / idc_api / idc_rccl / idc_diag .hip): the graph's
// types, the handle, the options, HIPCHK / fail() and the functions that cross a unit boundary.  Everything else is static in its unit.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/ideepcolor.h"
#include "idc_batch.h"
#include "idc_kernels.h"
#include "idc_layout.h"
#include "idc_mem.h"
#include "idc_net.h"

namespace idc {

// The 32x32x16-MFMA partners of the throughput kernels (conv_igemm_v2, conv_ds_fused, conv1_1_bf16_kernel: idc_v2.hip, idc_conv1.hip) exist only in the
// -DIDC_AB_PARTNERS build (round 6).  The default library plans every launch on conv_igemm_v2p / conv_igemm_v2m / conv_ds_fused_m / conv1_block_fused_t or
// the small-tile kernels, and refuses the option values that ask for a partner.
#ifdef IDC_AB_PARTNERS
static constexpr bool kAbPartners = true;
#else
static constexpr bool kAbPartners = false;
#endif

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Tensor {
    std::string name;
    void* ptr = nullptr;
    int C = 0, Cpad = 0, H = 0, W = 0;
    int is_f32 = 0;                      // fp32 storage (else the context's element type)
    int parts = 1;                       // operand-split precisions: bf16 planes per pixel ([part][Cpad]); 1 otherwise
    size_t bytes = 0;
};

// The launch_* conv entry point a layer runs (idc_kernels.h).  set_geometry sizes a launch for one of the tile families kConvIgemm,
// kConvClick, kConvWino, kDeconvWino, kConvKwave (the deconv form and the persistent trunk chain are reached through it) or kConvV2 (the
// large tile) and records it; choose_kernel then names the entry point, once per layer per forward, and everything after reads that.
enum Kernel {
    kConvIgemm, kConvClick, kConvWino, kDeconvWino, kConvKwave,      // launch_conv (+ splitk_epilogue), launch_conv_click, _conv_wino, _deconv_wino, _conv_kwave
    kConvV2, kConvV2m, kConvV2p, kConvV2s, kConvV2ps,                // the large tile: launch_conv_v2 (partner build), _v2m, _v2p (IDC_FP16: v2ph), _v2s, _v2ps
    kConvDs, kConvDsM, kConvDsMs,                                    // deconv + shortcut conv: launch_conv_ds (partner build), _ds_m (IDC_FP16: _mh), _ds_ms
    kConv1Block, kConv1_1Bf16, kConv1_1Split, kConv1_2Split,         // model1: launch_conv1_block, _conv1_1_bf16 (partner build), _conv1_1_split, _conv1_2_split
    kFused,                                                          // not launched: rides in another layer's launch (its fused_next / fused_short)
};

struct Layer {
    const LayerSpec* spec = nullptr;
    LayerBlob blob;
    int src = -1, dst = -1, resid = -1;
    int halo = 0;
    ConvConfig cfg{2, 2};
    Kernel kernel = kConvIgemm;          // the entry point this forward launches (plan_forward: set_geometry's tile family, then choose_kernel)
    int chain_len = 0;                   // > 0: this layer and the chain_len - 1 after it ran as ONE conv_kwave_chain_bf16 launch (last forward)
    int chained_into = -1;               // >= 0: ran inside the chain launch headed by that layer (last forward)
    bool fused_head = false;             // conv10_2 only: model_out + tanh run in this layer's epilogue
    bool shifted = false;                // conv4_3 under global hints: the branch's per-image vector is added in this layer's epilogue
    int fused_short = -1;                // deconv layers: index of the shortcut conv layer riding in this launch's K loop
    int fused_next = -1;                 // conv1_1 only: index of conv1_2 when model1 runs as one launch (conv1_block_fused)
    int lprec = 0;                       // the precision this layer's kernels run in (the handle's; IDC_FP32 on the fp32 island of a split handle)
    bool split = false;                  // operand-split launch (conv_igemm_v2s / conv_igemm_v2ps)
    ConvArgs args{};                     // zero-initialised; who writes which field: the table above plan_forward (idc_plan.hip)
    double flops = 0, min_bytes = 0;
};

// What a forward's plan is a function of, besides the layers, the tensors' shapes and options(): no pointer among it.
struct PlanEnv {
    int precision = 0;
    unsigned flags = 0;
    int H = 0, W = 0, max_batch = 0, n = 0;      // max_batch: the batch the kernel variants are chosen for; n: the batch launched
    int t_conv10_2 = -1, t_conv4_3 = -1;         // tensor indices: the regression head's input, the global-hints shift's target (-1: not in this graph)
    const std::vector<float>* wscale = nullptr;  // accumulator-scale word per layer (operand-split blobs), or nullptr
};

// Where a launch's pointers come from: the parameter blob, the tensors and the call's I/O planes.
struct BindEnv {
    const uint8_t* blob = nullptr;
    size_t head_w_off = 0, head_b_off = 0;       // model_out's parameters in the blob
    const std::vector<Tensor>* tensors = nullptr;
    const void* zeros = nullptr;
    const float* glob_vec = nullptr;             // global hints: the branch's [N][512] output
    float* partial = nullptr;                    // split-K slice sums (the caller sized them for the layer it binds)
    const float *L = nullptr, *ab = nullptr, *mask = nullptr;      // the call's input planes ...
    float l_div = 100.f, ab_div = 110.f, mask_mul = 1.f, mask_cent = 0.f;
    float* out = nullptr; float out_mul = 110.f;                   // ... and its ab map
};

// The options of idc_set_option / idc_set_tile_policy / idc_set_splitk_policy (idc_plan.hip): one object per process, options().
struct Options {
    // Tile policy (speed only; every choice computes the same result): 0 = automatic, 1 = always the
    // small-tile kernels (conv_igemm), 2 = the large-tile bf16 kernel (conv_igemm_v2) wherever it applies.
    int tile_policy = 0;
    int fuse_conv1 = idc_env_int("IDC_FUSE_CONV1", 1) != 0;        // model1 (conv1_1 + conv1_2) as one launch on the bf16 throughput path (idc_set_option / env IDC_FUSE_CONV1=0 for A/B)
    // Split-K policy of the small-tile kernels (speed only): 0 = automatic (launches that would leave most CUs idle,
    // i.e. the batch-1 click path), 1 = never, 2 = always split as far as the cin chunks allow (tests).
    int splitk_policy = 0;
    // fp32 path: 3x3 stride-1 layers as Winograd F(2x2,3x3), small deconv launches as F(2x2,2x2) (idc_set_option "winograd"): 0 = off (direct kernels),
    // 1 = automatic (default), 2 = wherever the forms are implemented (deconvs at every size: tests), 12 / 21 / 22 = automatic with the 3x3 form
    // <TB,CB> forced (tests, tuning).  The bf16 twins of round 3 were retired in round 5 (docs/experiments/conv_wino_bf16_round3.hip.txt).
    int wino = 1;
    int wino_deconv = 1;                 // 1 = small launches with Cin >= 256 only; 2 = every deconv ("winograd" = 2)
    // conv_igemm_v2 launches that qualify run as conv_igemm_v2m (16x16x32 MFMA: fewer joules per FLOP at the power cap; idc_set_option "mfma16")
    int mfma16 = idc_env_int("IDC_MFMA16", 1);
    // ... and so do the three deconv + shortcut launches (conv_ds_fused_m, idc_dsm.hip; idc_set_option "ds_mfma16" / env IDC_DS_M16=0 for A/B)
    int ds_m16 = idc_env_int("IDC_DS_M16", 1);
    // operand-split precisions: the deconv + shortcut pairs as ONE launch (conv_ds_fused_ms / _msh) instead of shortcut conv (fp32 sums to HBM) + deconv
    // (idc_set_option "split_ds_fuse", 0 for A/B)
    int split_ds_fuse = 1;
    // ... and conv1_1, their exact-fp32 island, on conv1_1_split_kernel where the grid is throughput-sized (>= 128 tiles of 32 x 16; "conv1_1_split", 0 = conv_igemm<float>)
    int conv1_1_split = 1;
    // ... and conv1_2 (64 -> 64 at full resolution) on conv1_2_split_kernel instead of the generic 64-cout tile ("conv1_2_split", 0 = conv_igemm_v2ps<1,4,1>)
    int conv1_2_split = 1;
    // IDC_FP16 (one fp16 part, one segment): launches the bf16 throughput kernels cover run their fp16 twins (conv_igemm_v2ph, conv_ds_fused_mh: bias in the
    // accumulators, packed-pair epilogue) instead of the one-segment split kernels ("fp16_fast", 0 = the split kernels everywhere)
    int fp16_fast = 1;
    // ... and the 3x3 convs among them as conv_igemm_v2p (no address arithmetic in the K loop; idc_set_option "v2p" / env IDC_V2P=0 for A/B)
    int v2p = idc_env_int("IDC_V2P", 1);
    // throughput kernels touch their own code at entry (idc_warm_own_code, idc_kernels.h; env IDC_CODE_WARM=0 for the A/B of profiles/r04_firstuse.txt)
    int code_warm = idc_env_int("IDC_CODE_WARM", 1);
    // bf16 click path: the 3x3 stride-1 layers and the deconvs as conv_kwave_bf16 / conv_kwave_deconv_bf16 ("kwave"; 0 = conv_click + split-K, round 2's kernels)
    int kwave = 1;
    // ... and runs of consecutive same-shape 8-chunk conv_kwave_bf16 layers (the 512 -> 512 trunk at batch 1) as ONE persistent launch with a
    // grid barrier between layers ("kwave_chain" / IDC_KWAVE_CHAIN): 0 = off, 1 = hipLaunchCooperativeKernel (+24 us per launch on this runtime),
    // 2 = plain launch after an occupancy check (default; a workgroup that never sees the others gives up after ~0.3 s and the handle falls back)
    int kwave_chain = idc_env_int("IDC_KWAVE_CHAIN", 2);
    int spin_sync = 1;                   // one- and two-image calls poll the stream instead of parking on an interrupt ("spin_sync"; 0 = the blocking wait of rounds 1-4)
    int pcie_kernel = 1;                 // their host <-> device transfers as copy kernels on the forward's stream ("pcie_kernel"; 0 = hipMemcpyAsync / the copy engines)
    int kw_force_abort = 0;              // test hook ("kw_force_abort"): the persistent trunk launch's first grid barrier is unreachable and its give-up counter tiny
    // single-operator entry points (idc_diag.hip): the batch their kernel variant is chosen for, as a handle's max_batch is ("op_policy_batch"; 0 = the call's own batch)
    int op_policy_batch = 0;
    // ... and how they store: the output tensor in fp32 in every precision, LayerSpec.out_f32 set ("op_out_f32"); the shortcut sum of an IDC_BF16 op in
    // fp32 ("op_resid_f32") -- what the class / 313 logits and the hyper-column partial sums of the distribution heads are inside a network
    int op_out_f32 = 0;
    int op_resid_f32 = 0;
    int click = -1;                      // conv_click for small launches: -1 = environment default (on), 0 off, 1 on (idc_set_option "click")
};
Options& options();

}  // namespace idc

using namespace idc;

// Everything the handle takes from the runtime is held by an owner (idc_mem.h), so destroying the handle is `delete`.  Members go in reverse order of
// declaration: the streams are declared before every buffer and event, and so are destroyed after them.
struct idc_context {
    int device = 0, H = 0, W = 0, max_batch = 0, precision = 0;
    unsigned flags = 0;
    Stream stream;
    Stream s_in, s_out;                  // the transfer pipeline's copy-in and copy-out streams (ensure_pipeline)
    std::string err;
    float l_div = 100.f, ab_div = 110.f, mask_mul = 1.f, out_mul = 110.f;
    BlobPlan plan;
    const uint8_t* d_blob = nullptr;     // the parameter blob in use: blob_mem's, or the caller's (idc_set_weights_device without copy)
    DevMem<uint8_t> blob_mem;            // the handle's own copy (own_blob_storage); empty while the caller's is in use
    bool weights_set = false;
    std::vector<Tensor> tensors;
    std::vector<Layer> layers;
    int t_input = -1, t_conv10_2 = -1, t_logits = -1;
    // staging for the host-pointer forward
    PinnedMem<float> h_in, h_out, h_dist;
    DevMem<float> d_L, d_ab, d_mask, d_out, d_dist;
    DevMem<float> d_scratch;
    DevMem<float> d_partial;             // split-K slice sums (grown on demand)
    DevMem<void> d_zeros;                // 256 zero bytes: LDS-DMA source of out-of-image halo rows (conv_click)
    DevMem<unsigned long long> d_kw_bar;      // conv_kwave_chain_bf16's grid-barrier counter (monotone) ...
    unsigned long long kw_bar_count = 0;      // ... grid barriers done by every launch so far (each adds its arrivals to its counter)
    int kw_bar_blocks = 0;                    // ... workgroups per launch those counts are for (a different grid resets the counters)
    DevMem<long long> d_kw_stamps;            // IDC_KW_STAMPS=1: per-phase cycle stamps of the last chain launch, printed when the handle is destroyed
    int kw_stamp_layers = 0, kw_stamp_blocks = 0;
    PinnedMem<int> h_kw_abort{hipHostMallocMapped};   // pinned, device-visible: a chain workgroup that gave up waiting sets it
    bool kw_chain_off = false;                // set after a refused / aborted chain launch: the handle falls back to one launch per layer
    int kw_chain_fits = -1;                   // workgroups of the chain kernel this device holds at once (-1: not asked yet)
    DevMem<float> d_glob_in, d_glob_vec; // global hints: [max_batch][316] inputs, [max_batch][512] branch output
    int t_conv4_3 = -1, t_pred313 = -1;
    DevMem<float> d_pred_ab, d_dist313;  // 313 head outputs
    PinnedMem<float> h_pred_ab;
    float dist_S = 0.2f;
    DevMem<unsigned char> d_rgb;         // colour post-processing (allocated on first use)
    PinnedMem<unsigned char> h_rgb;
    DevMem<double> d_labq;
    PinnedMem<double> h_labq;
    DevMem<float> d_post_in;             // idc_lab2rgb staging (L + ab planes): the resident L / hint planes are left alone
    bool want_dist313 = false;           // the next forward also writes the full-resolution dist_S
    bool keep_dist313 = false;           // idc_keep_dist: every forward leaves dist_S resident (colour suggestions)
    int dist_n = 0;                      // images whose distribution is resident from the last forward (0 = none)
    DevMem<HintRect> d_hints;            // click session: hint list staging
    PinnedMem<HintRect> h_hints;
    DevMem<unsigned char> d_layer;       // idc_set_hints_layer: the one RGBA layer ...
    DevMem<unsigned char> d_layer_meta;  // ... its LayerDesc at 0 and the cell count int32 at 16 ...
    PinnedMem<unsigned char> h_layer_meta;    // ... and their pinned copy
    DevMem<unsigned char> d_reveal;      // idc_reveal_hints: the kept rectangles' places in the caller's list int[kept], then colours float[n_hints][2] ...
    PinnedMem<unsigned char> h_reveal;   // ... and their pinned copy
    DevMem<float> d_centres; DevMem<double> d_sugg; DevMem<unsigned> d_sugg_counts;   // colour suggestions
    DevMem<float> d_map_ab, d_map_s;     // idc_dist_decode / idc_dist_entropy results: [max_batch][2][npix], [max_batch][npix] (first use)
    // idc_dist_peaks / idc_suggest_colors_batch: one device block and one pinned block per call (the picker's work map, peaks and peak_ent; the
    // queries and centres in, the suggestions out), grown on demand: both calls block, so nothing is in flight when they grow
    DevMem<unsigned char> d_taps;
    PinnedMem<unsigned char> h_taps;
    DevMem<unsigned char> d_score;       // idc_dist_score: the centres and one block for what the score produces (ScoreLayout), grown on demand; the call blocks
    std::vector<char> l_set;             // per image slot: d_L holds an uploaded L plane (idc_forward_resident refuses otherwise)
    // image ingestion (idc_set_image_rgb / idc_fullres_rgb): per slot the uint8 source kept on the device (IDC_INGEST_KEEP_SOURCE; empty = none)
    // and its size, and the mask_value of the slot's last idc_set_hints (0 = never had hints)
    // ... and the l_cent of that ingestion: with the slot's L plane it is the guide of the joint upsampling (a source is resident only while that plane is intact)
    // ... and its format: gray_bits 0 = [h,w,3] uint8 RGB (idc_set_image_rgb), 8 | 16 = one plane [h,w] of uint8 | uint16 (idc_set_image_gray)
    // ... and, for a source that was down-scaled while the ingest filter was IDC_FILTER_ANTIALIAS, the net-size lattice image [H,W,3] / [H,W] the
    // pre-pass made of it (empty otherwise): what idc_reveal_hints and idc_dist_score read in place of the source
    struct SlotSource { DevMem<unsigned char> d_rgb, d_net; int h = 0, w = 0; float l_cent = 0.f; int gray_bits = 0; };
    std::vector<SlotSource> src;
    std::vector<float> hint_mask_value;
    DevMem<unsigned char> d_ingest;                                  // upload buffer of the sources that are not kept
    // antialiased ingestion (idc_set_ingest_filter; a pipelined call takes its copy when it is enqueued): the net-size images of a blocking call's
    // sources that are not kept, and the ResampleJob table of one pre-pass launch, device and pinned
    int ingest_filter = 0;               // IDC_FILTER_BILINEAR
    DevMem<unsigned char> d_aa, d_aa_jobs;
    PinnedMem<unsigned char> h_aa_jobs;
    DevMem<const unsigned char*> d_src_ptrs;                         // [max_batch] source pointers of one ingest launch ...
    PinnedMem<const unsigned char*> h_src_ptrs;                      // ... and their pinned host copy
    DevMem<unsigned char> d_net_rgb; DevMem<double> d_net_lab;       // idc_set_image_rgb results [max_batch,H,W,3] u8, [max_batch,3,H,W] f64 (first use)
    DevMem<unsigned char> d_full_rgb;    // idc_fullres_rgb result ...
    PinnedMem<unsigned char> h_full_rgb; // ... and (pageable callers) its pinned staging, as large
    DevMem<double> d_full_ab;            // idc_fullres_ab result [2,src_h,src_w] ...
    PinnedMem<double> h_full_ab;         // ... and its pinned staging
    // joint bilateral upsampling: idc_set_joint_upsample's parameters and idc_set_batch_upsample's interp; a pipelined call takes its copy when it is enqueued
    JointParams joint = {2, 2.0 * 1.0 * 1.0, 2.0 * 8.0 * 8.0};
    int batch_interp = 1;                // IDC_INTERP_LINEAR
    // YCbCr 4:2:0 output (idc_set_batch_output; a pipelined call takes its copy of the pair when it is enqueued), and what the two blocking calls
    // work in: idc_fullres_ycc's / idc_rgb_to_ycc420's packed plane blocks, the YccDesc table of one launch and idc_rgb_to_ycc420's packed RGB,
    // device and pinned, grown on demand: both calls block, so nothing is in flight when they grow
    int out_format = 0, out_matrix = 0;  // IDC_OUT_RGB, IDC_YCC_JFIF
    DevMem<unsigned char> d_ycc, d_ycc_meta, d_ycc_in;
    PinnedMem<unsigned char> h_ycc, h_ycc_meta, h_ycc_in;
    // temporal ab filter (idc_set_temporal_filter; a pipelined call takes its copy of the parameters when it is enqueued): the sequence state
    // y_prev [2,H,W] and l_prev [H,W] fp32 on the device, whether a frame has been ENQUEUED since idc_create / idc_temporal_reset (every launch
    // that reads or writes the state is on the compute stream, so the host's flag at enqueue time is the device's truth at run time), and what
    // the blocking idc_temporal_apply works in: its frames, the two kernels' scratch and its info block, grown on demand
    TemporalParams temporal = temporal_defaults();
    bool temporal_have = false;
    DevMem<float> d_t_yprev, d_t_lprev, d_t_x, d_t_l;
    DevMem<unsigned char> d_t_scratch, d_t_info;
    // its motion compensation (idc_set_temporal_motion; copied into a pipelined call like the filter's parameters), and what idc_temporal_apply
    // leaves for idc_temporal_vectors(-1): the vectors of its last call (device scratch and the host's copy), its frame count (0: no call yet)
    // and whether it ran with motion on
    MotionParams motion = motion_defaults();
    DevMem<unsigned char> d_t_vec;
    std::vector<int8_t> t_apply_vec;
    int t_apply_n = 0;
    bool t_apply_motion = false;
    // the hint tracking along those vectors (idc_set_hint_tracking; copied into a pipelined call like the motion parameters): the sequence state
    // (A, M, G) of the last tracked frame in idc_track.h's one-frame layout, whether it holds a frame (a tracking call has been ENQUEUED since
    // idc_create / idc_temporal_reset and no filtered call without tracking since), and what the blocking idc_track_hints_apply works in
    TrackParams track = track_defaults();
    bool track_have = false;
    DevMem<unsigned char> d_tr_state, d_tr_in, d_tr_out;
    DevMem<unsigned char> d_pick;       // idc_gamut_map / idc_snap_colors: inputs + results of one call, device and pinned
    PinnedMem<unsigned char> h_pick;
    Event ev_sync;                       // idc_stream_wait / idc_stream_signal
    // reference-image global hints (idc_global_stats_rgb / idc_set_global_refs; one per pipeline slot for idc_forward_async_rgb_ref): what one
    // call sends -- the RefDesc table, the reference index, the centres and the packed uint8 references as ONE block, pinned and device -- and
    // what its kernels work in: counts, per-workgroup saturation sums, and the histograms / mean saturations a caller asked for (RefLayout)
    struct RefStage {
        PinnedMem<unsigned char> h_in, h_res;
        DevMem<unsigned char> d_in, d_work;
    };
    RefStage ref;
    // two-slot transfer pipeline (idc_forward_async / idc_wait): each slot owns its device planes
    struct PipeSlot {
        DevMem<float> d_L, d_ab, d_mask, d_out;                                        // device I/O planes
        PinnedMem<float> h_in, h_out;                                                  // pinned staging (pageable callers)
        Event ev_in, ev_comp, ev_out;
        Event ev_in0, ev_comp0, ev_out0;                                               // stage starts (idc_pipeline_times)
        bool pending = false, timed = false;
        int up_interp = 1; JointParams up_joint = {2, 2.0, 128.0};                     // the source-size upsampling the batch in flight was enqueued with
        int ingest_filter = 0;                                                         // ... and the ingest filter
        // what idc_wait still has to copy to a pageable destination of the batch in flight: `bytes` from the slot's pinned memory, where the
        // copy-out stream left them (one entry per pageable buffer of the call, whatever it holds; a pinned destination was written in place)
        struct StagedOut { void* user; const void* pinned; size_t bytes; };
        std::vector<StagedOut> outs;
        // idc_forward_async_rgb: the batch's packed uint8 source, its metadata block (BatchPlan, idc_batch.h), the net-size result, the
        // refreshed Lab and the source-size result (IDC_BATCH_OUT_SOURCE); grown on demand
        DevMem<unsigned char> d_src, d_meta, d_rgb, d_full;
        DevMem<double> d_labq;
        PinnedMem<unsigned char> h_src, h_meta, h_rgb;                                 // pinned staging: pageable sources, the block, pageable rgb_out
        // idc_forward_async_eval: the net-size ground truth [max_batch,H,W,3] (a net-size score), and one block for what the batch reports
        // (BatchPlan: sse, then hint_colours), on the device and pinned
        DevMem<unsigned char> d_truth, d_eval;
        PinnedMem<unsigned char> h_eval;
        // idc_forward_async_dist: the taps' inputs (queries, centres) and one block for what they produce (TapsLayout), each device and pinned
        DevMem<unsigned char> d_taps_in, d_taps;
        PinnedMem<unsigned char> h_taps_in, h_taps;
        // idc_forward_async_dist_score: the centres and the score's result block (ScoreLayout), as for the taps
        DevMem<unsigned char> d_score_in, d_score;
        PinnedMem<unsigned char> h_score_in, h_score;
        // idc_forward_async_rgb_ref: the batch's references and the slot's OWN [max_batch][316] global inputs (the handle's d_glob_in is not touched)
        RefStage ref;
        DevMem<float> d_glob_in;
        // idc_forward_async_layers: the batch's packed RGBA layers (BatchPlan::layer_pieces) and the cell counts int32[max_batch], device and pinned
        DevMem<unsigned char> d_layer, d_cells;
        PinnedMem<unsigned char> h_layer, h_cells;
        // idc_set_batch_output: the batch's packed plane blocks (BatchPlan::ycc_bytes), which leave the device in place of d_rgb / d_full
        DevMem<unsigned char> d_ycc;
        // idc_set_temporal_filter: the parameters the slot's last call was enqueued with (on = 0: it ran unfiltered), its frame count, the two
        // kernels' scratch (idc_temporal.h) and the info block D [n] + cut [n], device and pinned: it always travels back, it is small
        TemporalParams temporal = temporal_defaults();
        int temporal_n = 0;
        DevMem<unsigned char> d_t_scratch, d_t_info;
        PinnedMem<unsigned char> h_t_info;
        // idc_set_temporal_motion: what the slot's last call was enqueued with, and its vectors (idc_motion.h), device and pinned: they travel
        // back with the info block, only when motion was on
        MotionParams motion = motion_defaults();
        DevMem<unsigned char> d_t_vec;
        PinnedMem<unsigned char> h_t_vec;
        // idc_set_hint_tracking: whether the slot's last call tracked its hints, with what, and the tracked planes (idc_track.h) the network
        // and the taps then read in place of d_ab / d_mask; idc_tracked_hints copies from here on request
        bool tracked = false;
        TrackParams track = track_defaults();
        DevMem<unsigned char> d_tr;
    } pipe[2];
    Event ev_pipe_base;
    bool pipe_ready = false;             // ev_pipe_base is recorded (ensure_pipeline)
    DevMem<unsigned char> d_up_rgb; DevMem<double> d_up_L;           // idc_upsample_lab2rgb staging
    PinnedMem<unsigned char> h_up_rgb; PinnedMem<double> h_up_L;
    bool out_copy_pending = false;       // forward_host(finish = false): the ab map still has to be copied from h_out to the caller
    bool out_resident = false;           // d_out / d_labq hold the last forward's ab map / refreshed Lab
    bool labq_resident = false;
    int profiling = 0;                   // 0 off, 1 = an event pair around every launch, 2 = one pair around the whole forward
    DevMem<void> d_arena;                // all activation tensors (alloc_graph) ...
    std::vector<DevMem<void>> tensor_mem;    // ... or one allocation per tensor with IDC_ARENA=0; Tensor::ptr views either
    std::vector<Event> ev;               // kProfRing slots x 2 per timed step: [pack, layers..., head, softmax]
    int n_timed = 0;
    long long prof_count = 0;            // forwards recorded since profiling was switched on
    int last_n = 0;
    // range audit (idc_set_range_audit): one sticky AuditRecord per row of the layer table in device memory, the value counts on the host
    bool audit = false;
    DevMem<AuditRecord> d_audit;
    std::vector<unsigned long long> audit_values;
    // from the blob in use (cache_blob_meta): the activation exponent of each active layer's output and its accumulator-scale word
    std::vector<int> act_exp;
    std::vector<float> wscale;
};

#define HIPCHK(ctx, expr)                                                                                  \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) (void)hipGetLastError();   /* reported through our own status: do not leave it sticky for the caller's runtime */ \
        if (e_ != hipSuccess)                                                                              \
            return fail((ctx) ? &(ctx)->err : nullptr, IDC_ERR_HIP, "%s failed: %s (%s:%d)", #expr,        \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                        \
    } while (0)

namespace idc {

static constexpr int kProfRing = 32;    // per-layer event pairs are kept for the last 32 forwards

// idc_api.hip (which also owns the thread-local last-error string: fail() writes it, idc_last_error() reads it)
int fail(std::string* err, int code, const char* fmt, ...);
int check_device(int device_id, std::string* err);
int ensure_post_buffers(idc_context* h);
int run_lab_post(idc_context* h, int n, const float* d_Lp, float l_add, const float* d_abp, uint8_t* rgb, double* lab_q);
void drop_source(idc_context* h, int slot);      // the slot's L plane is about to be overwritten by something else than idc_set_image_rgb: its resident source goes

// idc_pack.hip (make_blob_plan: idc_net.h)
int f16_weight_exponent(const float* w, size_t n);
void pack_layer_weights(uint8_t* wimg, int precision, int layout, const LayerSpec& s, const LayerBlob& lb, const float* w, int part = 0, float wmul = 1.f);
void pack_wino_weights(uint8_t* img, int precision, const LayerSpec& s, const LayerBlob& lb, const float* w);
void pack_wino_deconv_weights(uint8_t* img, int precision, const LayerSpec& s, const LayerBlob& lb, const float* w);
int verify_device_blob(idc_context* h, const void* dev_blob, size_t blob_bytes);
int own_blob_storage(idc_context* h);            // d_blob = the handle's own allocation of plan.total_bytes, made unless it already has one

// idc_plan.hip
int find_tensor(const std::vector<Tensor>& tensors, const char* name);
void fill_taps(Layer& L);
int plan_forward(std::vector<Layer>& layers, const std::vector<Tensor>& tensors, const PlanEnv& env, std::string* err);
hipError_t launch_kernel(Kernel k, const Layer& L, const ConvArgs& a, hipStream_t s);
void kernel_label(const Layer& L, int precision, char* out, size_t cap);
int build_layers(const BlobPlan& plan, int precision, int H, int W, int max_batch, std::vector<Tensor>& tensors, std::vector<Layer>& layers, std::string* err);
int check_geometry(int precision, unsigned flags, int H, int W, int max_batch, std::string* err);
int build_graph(idc_context* c);
int alloc_graph(idc_context* c);

// idc_exec.hip
void bind_layer(std::vector<Layer>& layers, int li, const BindEnv& env);
// glob_in: the [n][316] global-input block the Global-Hints branch reads (the handle's d_glob_in, or a pipeline slot's own); unused without the branch
int run_graph(idc_context* c, int n, const float* dL, const float* dab, const float* dmask, float maskcent, float* dout, float* ddist,
              const float* glob_in);
// reference-image global hints: where each part of a call sits in RefStage's blocks (byte offsets; the RefDesc table is at 0 of the input block,
// the counts at 0 of the work block)
struct RefLayout {
    int n = 0, m = 0;                    // images that take a row (0: idc_global_stats_rgb), references
    size_t o_index = 0, o_centres = 0, o_packed = 0, in_bytes = 0, ref_bytes = 0;
    size_t o_sat = 0, o_hist = 0, o_savg = 0, work_bytes = 0;
    // antialiased ingestion (check_refs with the handle's filter on and at least one down-scaled reference; naa = 0 otherwise, and every byte
    // above is today's): the ResampleJob table [naa] at o_jobs, behind the packed references and uploaded with them, and the net-size images
    // [naa,H,W,3] the pre-pass writes at o_aa of the same device block (never uploaded); the RefDesc of such a reference points there
    int naa = 0, aa_tiles = 0;
    size_t o_jobs = 0, o_aa = 0, up_bytes = 0, dev_bytes = 0;
};
// every check of the reference arguments (include/ideepcolor.h's table), on the host, before anything is allocated or enqueued; m_min = 0 or 1
int check_refs(idc_context* c, int m_min, int n, int m, const idc_ref_image* refs, const int32_t* ref_index, const float* centres,
               float hist_flag, unsigned ref_flags, RefLayout* lay);
// grow the stage (the caller knows nothing of it is in flight) and copy table, index, centres and references into its pinned block
int stage_refs(idc_context* c, idc_context::RefStage& st, const RefLayout& lay, const idc_ref_image* refs, const int32_t* ref_index,
               const float* centres, bool want_results);
// one H2D copy of the input block on `copy`; then on `s`: counts zeroed, ref_stats_kernel, glob_rows_kernel into rows (n rows; may be nullptr
// with n == 0) and, with want_hist, the stage's hist / s_avg section
int upload_refs(idc_context* c, idc_context::RefStage& st, const RefLayout& lay, hipStream_t copy);
int launch_refs(idc_context* c, idc_context::RefStage& st, const RefLayout& lay, float hist_flag, unsigned ref_flags, float* rows, bool want_hist,
                hipStream_t s);
// distribution taps (idc_dist_peaks / idc_suggest_colors_batch / idc_forward_async_dist): the geometry of the handle's distribution, every check of
// include/ideepcolor.h's table on the host, and where each part sits in the input and result blocks (byte offsets, 16-byte aligned)
struct DistGeom { int B = 0, Hd = 0, Wd = 0, s = 1; const float* dist = nullptr; };
struct TapsLayout {
    int n = 0, P = 0, Q = 0, K = 0;      // Q: suggestion rows (the query count, or n * P at the peaks)
    bool at_peaks = false, want_ent = false;
    size_t i_centres = 0, in_bytes = 0;                                        // input block: DistQuery[n_queries], then centres float[B][2]
    size_t o_ent = 0, o_work = 0, o_peaks = 0, o_pent = 0, o_sc = 0, o_sf = 0, out_bytes = 0;
};
bool dist_geom(const idc_context* c, DistGeom* g);       // false: the handle has no distribution head that writes a distribution
int check_taps(idc_context* c, const DistGeom& g, int n, int p_min, int q_min, const idc_dist_taps* taps, TapsLayout* lay);
// on `s`: [entropy] [peaks, mask = the planes IDC_PEAKS_SKIP_HINTS reads] [suggestions] from `in` (device input block) into `out` (device result block)
int launch_taps(idc_context* c, const DistGeom& g, const TapsLayout& lay, const idc_dist_taps* taps, const float* mask, const unsigned char* in,
                unsigned char* out, hipStream_t s);
// distribution scores (idc_dist_score / idc_forward_async_dist_score): every check of include/ideepcolor.h's table on the host, and where each part
// sits in the result block (byte offsets, 16-byte aligned; the block sums come first and stay on the device, a map nobody asked for takes no room)
struct ScoreLayout {
    int n = 0, nn = 0;
    float sigma = 0.f;
    ScoreRanks ranks = {};
    bool want_xmap = false, want_rmap = false, want_tgt = false;
    size_t o_part = 0, o_xent = 0, o_hits = 0, o_truth = 0, o_xmap = 0, o_rmap = 0, o_tgt = 0, out_bytes = 0;
};
int check_score(idc_context* c, const DistGeom& g, int n, const idc_dist_score_spec* spec, const float* centres, const idc_dist_score_out* out,
                ScoreLayout* lay);
// on `s`: the score of truth (at lay.o_truth of `out`, written by launch_dist_truth before) into the device result block `out`
int launch_score(idc_context* c, const DistGeom& g, const ScoreLayout& lay, const float* centres, unsigned char* out, hipStream_t s);
int check_chain_abort(idc_context* c);
int check_forward_args(idc_context* c, int n);
hipError_t wait_stream(idc_context* c, int n);
hipError_t copy_h2d_or_d2h(idc_context* c, void* dev, void* host, size_t bytes, bool to_device);
bool is_pinned(const void* p);
int drain_pipeline(idc_context* c);

// idc_diag.hip
void layer_row(const std::vector<Layer>& layers, const std::vector<Tensor>& tensors, int precision, unsigned flags, int H, int W, int layer, idc_layer_info* out);

}  // namespace idc
