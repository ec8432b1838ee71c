// idc_plan.hip -- the graph planner: the static schedule of the SIGGRAPHGenerator graph (build_layers, build_graph, alloc_graph), the plan of one
// forward (plan_forward: tile family and launch geometry per layer -- set_geometry --, the fusions, the entry point each launch runs -- choose_kernel;
// launch_kernel and kernel_label read that choice), and the options that steer those choices (options(), idc_set_option, idc_set_tile_policy,
// idc_set_splitk_policy).  Nothing from build_layers to plan_forward touches the device: tools/plan_dump.cpp prints a configuration's plan without one.
#include <stdio.h>
#include <string.h>

#include "idc_engine.h"

namespace idc {

Options& options() { static Options o; return o; }

int find_tensor(const std::vector<Tensor>& tensors, const char* name) {
    for (size_t i = 0; i < tensors.size(); ++i)
        if (tensors[i].name == name) return (int)i;
    return -1;
}

static bool conv1_2_split_layer(const LayerSpec& s) {
    return s.kind == kConv3x3 && s.cin == 64 && s.cout == 64 && s.dilation == 1 && s.in_stride == 1 && s.act == 1 && !s.resid;
}

// Shortcut fusion (conv_igemm_v2<.,.,1,true>) is correct (parity-tested under tile policy 2) but measured slower
// than two launches on MI355X (4x re-reads of the skip tensor by the four phase workgroups, VGPR spills around
// the staged K loop): 0.87 ms -> 1.25 ms at level 1.  Off unless the tile policy forces every variant on.
// large-tile deconv launches also run the shortcut conv they are summed with (conv_ds_fused); IDC_FUSE_SHORTCUT=0 keeps
// the two launches apart (A/B)
static bool fuse_shortcut_enabled() {
    static const bool off = idc_env_int("IDC_FUSE_SHORTCUT", 1) == 0;
    return !off;
}

// Small-tile kernel shape.  cout<=64 layers can only use one 64-wide cout group per wave column;
// otherwise prefer 128 couts x 128 pixels and fall back to smaller pixel tiles when the launch would
// not fill the 256 CUs.
// Tuning knobs of the small-tile path (speed only), read once from the environment: tools/click_sweep.py walks them on
// the GPU box and the defaults below are what it found best (profiles/r02_click_sweep.txt).
static int env_int(const char* name, int dflt) { return idc_env_int(name, dflt); }      // (defaults only, unless built with -DIDC_AB_PARTNERS)
struct SmallTileTuning {
    int tiles_goal = env_int("IDC_ST_TILES_GOAL", 512);         // shrink the pixel tile until this many workgroups exist
    int force_wp = env_int("IDC_ST_FORCE_WP", 0);               // 1/2/4: fixed rows-of-4 per workgroup (0 = automatic)
    int force_wm = env_int("IDC_ST_FORCE_WM", 0);               // 1/2: cout groups per workgroup (0 = automatic)
    int sk_below[2] = {env_int("IDC_SK_BELOW_FP32", 256), env_int("IDC_SK_BELOW_BF16", 128)};   // split K when fewer tiles than this
    int sk_goal[2] = {env_int("IDC_SK_GOAL_FP32", 512), env_int("IDC_SK_GOAL_BF16", 256)};      // ... until about this many workgroups
    int v2_min_blocks = env_int("IDC_V2_MIN_BLOCKS", 128);      // large-tile bf16 kernel from this many workgroups on
    int v2_half_tiles = env_int("IDC_V2_HALF_TILES", 1);        // 4-wave large tiles for grids of 128..255 workgroups
    int v2_force22 = env_int("IDC_V2_FORCE22", 0);
    int v2_22_nkc = env_int("IDC_V2_22_NKC", 2);
    int click = env_int("IDC_CLICK", 1);                        // conv_click for small launches (the batch-1 click path)
    int click_max_wgs = env_int("IDC_CLICK_MAX_WGS", 1024);     // ... when its grid has at most this many workgroups
    int click_goal = env_int("IDC_CLICK_GOAL", 512);            // ... split K over the cin chunks until about this many exist (same-box A/B: 512 beats 256 by 1.5 % bf16 / 3 % fp32)
    int click_wp = env_int("IDC_CLICK_WP", 4);                  // rows-of-4 per workgroup (4 = 16x16 sites, 256 threads)
};
static const SmallTileTuning& tuning() { static const SmallTileTuning t; return t; }

static ConvConfig choose_config(int n, int Hs, int Ws, int coutpad, int nphase) {
    const SmallTileTuning& tn = tuning();
    int wm = coutpad >= 128 ? 2 : 1;
    if (tn.force_wm && coutpad >= 64 * tn.force_wm && (coutpad / 64) % tn.force_wm == 0) wm = tn.force_wm;
    if (tn.force_wp == 1 || tn.force_wp == 2 || tn.force_wp == 4) return ConvConfig{wm, tn.force_wp};
    const int cand_wp[3] = {wm == 1 ? 4 : 2, 2, 1};
    ConvConfig best{wm, cand_wp[0]};
    for (int i = 0; i < 3; ++i) {
        const int wp = cand_wp[i];
        const long long tiles = (long long)((Ws + 15) / 16) * ((Hs + 4 * wp - 1) / (4 * wp)) * n * (coutpad / (64 * wm)) * nphase;
        best = ConvConfig{wm, wp};
        if (tiles >= tn.tiles_goal) break;
    }
    return best;
}

void fill_taps(Layer& L) {
    ConvArgs& a = L.args;
    const LayerSpec& s = *L.spec;
    memset(a.dy, 0, sizeof(a.dy)); memset(a.dx, 0, sizeof(a.dx)); memset(a.tw, 0, sizeof(a.tw));
    memset(a.ro, 0, sizeof(a.ro)); memset(a.co, 0, sizeof(a.co));
    if (s.kind == kConv3x3) {
        a.nphase = 1; a.ntaps = 9; a.so = 1; a.si = s.in_stride;
        for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) {
                const int t = ky * 3 + kx;
                a.dy[t] = (ky - 1) * s.dilation; a.dx[t] = (kx - 1) * s.dilation; a.tw[t] = t;
            }
        L.halo = s.dilation;
    } else if (s.kind == kDeconv4x4) {
        // out[co,2m+r,2n+s] = b + sum over (ky,dy) in T(r), (kx,dx) in T(s) of in[m+dy,n+dx]*W[ci,co,ky,kx]
        // T(0) = {(1,0),(3,-1)}, T(1) = {(0,+1),(2,0)}     
        static const int T_k[2][2] = {{1, 3}, {0, 2}};
        static const int T_d[2][2] = {{0, -1}, {1, 0}};
        a.nphase = 4; a.ntaps = 4; a.so = 2; a.si = 1;
        for (int r = 0; r < 2; ++r)
            for (int c = 0; c < 2; ++c) {
                const int ph = r * 2 + c;
                a.ro[ph] = r; a.co[ph] = c;
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 2; ++j) {
                        const int t = ph * 9 + i * 2 + j;
                        a.dy[t] = T_d[r][i]; a.dx[t] = T_d[c][j];
                        a.tw[t] = T_k[r][i] * 4 + T_k[c][j];
                    }
            }
        L.halo = 1;
    } else {
        a.nphase = 1; a.ntaps = 1; a.so = 1; a.si = 1;
        L.halo = 0;
    }
}

// n_policy: the batch the kernel variant is chosen for (the handle's max_batch, so that a handle's
// numerics do not depend on how many images a call carries); n: the batch actually launched.
static void set_geometry(Layer& L, int precision, int n, int n_policy, int Hs, int Ws, bool allow_v2) {
    const Options& o = options();
    ConvArgs& a = L.args;
    a.N = n; a.Hs = Hs; a.Ws = Ws;
    a.nkc = L.blob.nkc; a.ncg = L.blob.ncg;
    a.act = L.spec->act;
    // fp32 path: every 3x3 stride-1 layer whose U image is in the blob runs as Winograd F(2x2,3x3): 2.25x fewer multiplies
    // on the exact-fp32 matrix pipe, no split-K at batch 1 (one workgroup per 16 tiles x 32 couts)
    bool wino = precision == IDC_FP32 && o.wino && o.tile_policy != 1 && L.blob.w3_off != (size_t)-1 &&
             (L.spec->kind == kDeconv4x4
                  ? (o.wino_deconv == 2 || (o.wino_deconv == 1 && a.nkc >= 8 &&
                                            (long long)((Ws + 7) / 8) * ((Hs + 7) / 8) * n_policy * (a.ncg * 4) <= 1024))
                  : L.spec->resid == nullptr);
    // (deconvs: only the small launches of the click path with Cin >= 256 -- the form is transform-bound (one 16-cout block per
    //  workgroup at the 168-register budget of its 12 waves): model10up (4 chunks) 123 us vs 96 us direct at batch 1, and at N = 32
    //  model8up / model9up 1.30 / 1.54 ms vs 1.23 / 1.31 ms direct; "winograd_deconv" = 2 forces it everywhere for the tests)
    const bool wino_fits = wino_offsets_fit(Hs, Ws, L.spec->kind == kDeconv4x4 ? 1 : L.spec->in_stride, a.nkc);   // 32-bit patch offsets
    wino = wino && wino_fits;
    if (wino) { L.kernel = L.spec->kind == kDeconv4x4 ? kDeconvWino : kConvWino; a.ksplit = 1; a.kc_per = a.nkc; a.tiles_x = a.tiles_y = 0; return; }
    // large-tile bf16 kernel: 256 couts x (32x8 sites) when the cout groups divide by 4, else
    // 128 couts x (32x16 sites); used when its grid covers at least half of the 256 CUs
    const bool split = is_split(precision);      // operand-split precisions: a throughput path, the large tile on every layer whatever the grid
    // (default library: fp32-output launches -- class_logits -- stay on the small tile: conv_igemm_v2m / v2p write bf16 only)
    const bool v2_covers = allow_v2 && (kAbPartners || !L.spec->out_f32);
    if (split ? !split_island(*L.spec) : (precision == IDC_BF16 && v2_eligible(*L.spec) && o.tile_policy != 1 && v2_covers)) {
        ConvConfig c2 = (a.ncg % 4 == 0) ? ConvConfig{4, 2} : (a.ncg % 2 == 0) ? ConvConfig{2, 4} : ConvConfig{1, 4};   // ({1,*}: split precisions only, conv1_2)
        int tx = (Ws + 31) / 32, ty = (Hs + 4 * c2.wp - 1) / (4 * c2.wp);
        long long blocks = (long long)tx * ty * n_policy * (a.ncg / c2.wm) * a.nphase;
        // between one half and one full wave of workgroups (batch-1 conv10_2: 128 tiles on 256 CUs): the 4-wave tile
        // 128 couts x (32 x 8 sites) doubles the grid
        // ... and the same 4-wave tile wherever a CU walks several tiles with a short K loop each (128-cout layers, and
        // layers with <= v2_22_nkc cin chunks): two 4-wave workgroups share a CU (75.5 KiB of LDS each) and run out of
        // step, so one's prologue / epilogue hides under the other's MFMAs.  Same-box A/B at N = 32 (profiles/
        // r02_tile22_ab.txt): conv10_2 -9.5 %, conv2_1 -8..14 %, conv2_2 -6 %, conv9_2 -6..12 %, conv3_1 -22 %; the
        // 512->512 trunk (one tile per CU, long K) is 1-2 % (dilated: 15 %) slower with it and keeps the 8-wave tile.
        const int force22 = tuning().v2_force22;     // experiment switch: 0 = rule above, 1 = never, 2 = everywhere
        // (the 64-cout tile of the split precisions keeps 32 x 16 sites: conv1_2 0.84 ms as {1,4}, 1.01 ms as {1,2} at N = 32, bf16x3)
        const bool rule22 = force22 == 2 || (force22 == 0 && (c2.wm == 2 || (c2.wm == 4 && a.nkc <= tuning().v2_22_nkc)) && blocks >= 256);
        // operand-split precisions have no batch-1 kernels: a grid that leaves most of the chip idle (fp16x3 at 1..8 images: the 512 -> 512 trunk is 8 x N
        // workgroups of the 8-wave tile) at least takes the 4-wave 128-cout tile -- twice the workgroups, half the K-loop time each (round 6, tools/batch_sweep.py)
        const bool split_small = split && blocks < 128;         // (at 128 workgroups -- the trunk at N = 16 -- the 8-wave tile is still the faster one: 2546 against 2475 img/s)
        if (a.nphase == 1 && c2.wm != 1 && ((blocks >= tuning().v2_min_blocks && blocks < 256 && tuning().v2_half_tiles) || rule22 || split_small)) {
            c2 = ConvConfig{2, 2};
            ty = (Hs + 4 * c2.wp - 1) / (4 * c2.wp);
            blocks = (long long)tx * ty * n_policy * (a.ncg / c2.wm) * a.nphase;
        }
        if (split || o.tile_policy == 2 || blocks >= tuning().v2_min_blocks) {
            L.kernel = kConvV2; L.cfg = c2; a.tiles_x = tx; a.tiles_y = ty;
            a.ksplit = 1; a.kc_per = a.nkc;
            return;
        }
    }
    // batch-1 click path: small launches are chains of exposed memory round trips in conv_igemm's K loop; conv_click
    // requests a workgroup's whole K slice at entry (as many cin chunks as fit in LDS next to their halo tiles)
    // ... "small" = fewer than v2_min_blocks big tiles (the criterion that hands a layer to the throughput kernels, applied to
    // every precision and cout width): conv_igemm's ring loop is the better kernel once the K loop is long and the chip full
    const int wm_big = a.ncg % 4 == 0 ? 4 : (a.ncg % 2 == 0 ? 2 : 1), rows_big = wm_big == 4 ? 8 : 16;
    const long long big_tiles = (long long)((Ws + 31) / 32) * ((Hs + rows_big - 1) / rows_big) * n_policy * (a.ncg / wm_big) * a.nphase;
    // bf16 click path, deconvs: the direct form with K split over the waves of a workgroup (conv_kwave_deconv_bf16, idc_kw.hip)
    if (precision == IDC_BF16 && o.kwave && o.tile_policy != 1 && big_tiles < tuning().v2_min_blocks && wino_fits &&
        L.spec->kind == kDeconv4x4 && (a.nkc == 2 || a.nkc == 4 || a.nkc == 8)) {
        L.kernel = kConvKwave; a.ksplit = 1; a.kc_per = a.nkc; a.tiles_x = a.tiles_y = 0;
        return;
    }
    // bf16 click path, 3x3 stride-1 layers: the direct form with K split over the waves of a workgroup (idc_kw.hip) -- 9/16 of the Winograd
    // form's weight stream, no reduction launch either
    if (precision == IDC_BF16 && o.kwave && o.tile_policy != 1 && big_tiles < tuning().v2_min_blocks && wino_fits && L.spec->resid == nullptr &&
        L.spec->kind == kConv3x3 && (a.nkc == 1 || a.nkc == 2 || a.nkc == 4 || a.nkc == 8)) {
        L.kernel = kConvKwave; a.ksplit = 1; a.kc_per = a.nkc; a.tiles_x = a.tiles_y = 0;
        return;
    }
    if ((o.click < 0 ? tuning().click : o.click) && o.tile_policy != 1 && big_tiles < tuning().v2_min_blocks &&
        (L.spec->kind == kConv3x3 || L.spec->kind == kDeconv4x4)) {
        int wp = tuning().click_wp;
        while (wp > 1 && 4 * wp > Hs * 2) wp >>= 1;               // tiny images: do not launch mostly-empty tiles
        const int maxc = conv_click_max_chunks(wp, L.halo, a.ntaps);
        const int tx = (Ws + 15) / 16, ty = (Hs + 4 * wp - 1) / (4 * wp);
        const long long tiles = (long long)tx * ty * n_policy * a.ncg * a.nphase;
        if (maxc >= 1) {
            int kc_per = maxc < a.nkc ? maxc : a.nkc;                         // split-K policy "never": one workgroup walks all chunks
            if (o.splitk_policy == 0)
                while (kc_per > 1 && tiles * ((a.nkc + kc_per - 1) / kc_per) < tuning().click_goal) --kc_per;
            if (o.splitk_policy == 2) kc_per = 1;
            if (kc_per >= 1) {
                const int ks = (a.nkc + kc_per - 1) / kc_per;
                if (tiles * ks <= tuning().click_max_wgs) {
                    L.kernel = kConvClick; L.cfg = ConvConfig{1, wp};
                    a.tiles_x = tx; a.tiles_y = ty; a.kc_per = kc_per; a.ksplit = ks;
                    return;
                }
            }
        }
    }
    L.kernel = kConvIgemm;
    L.cfg = choose_config(n_policy, Hs, Ws, L.blob.ncg * kCoutGroup, a.nphase);
    a.tiles_x = (Ws + 15) / 16;
    a.tiles_y = (Hs + 4 * L.cfg.wp - 1) / (4 * L.cfg.wp);
    // split-K: a launch of < 256 workgroups (batch-1: 32..128) cannot fill 256 CUs and each workgroup walks all
    // 9*Cin/64 tap-steps alone; cut the cin chunks into slices until ~512 workgroups exist
    a.ksplit = 1; a.kc_per = a.nkc;
    const long long tiles = (long long)a.tiles_x * a.tiles_y * n_policy * (a.ncg / L.cfg.wm) * a.nphase;
    const int pi = precision == IDC_FP32 ? 0 : 1;
    if (o.splitk_policy != 1 && a.nkc >= 2 && (o.splitk_policy == 2 || tiles < tuning().sk_below[pi])) {
        // fp32 tap-steps are 16x longer than bf16 ones: worth twice as many slices (measured: 3.0 -> 2.0 ms at N=1)
        long long want = o.splitk_policy == 2 ? a.nkc : (tuning().sk_goal[pi] + tiles - 1) / tiles;
        if (want > a.nkc) want = a.nkc;
        if (want >= 2) {
            a.kc_per = (int)((a.nkc + want - 1) / want);
            a.ksplit = (a.nkc + a.kc_per - 1) / a.kc_per;          // every slice is non-empty
            if (a.ksplit < 2) { a.ksplit = 1; a.kc_per = a.nkc; }
        }
    }
}

// The entry point a layer launches this forward: set_geometry's tile family (L.kernel) refined by the fusions planned on the layer, its
// arguments `a` as they will be bound (args_as_bound) and the options.  An exclusive chain in precedence order; where an entry point covers only
// some launches, its predicate decides here, so the launch that follows is never refused (a refusal is a planning bug: run_graph / run_single_op report it).
// max_batch: the batch the variant is chosen for (as set_geometry's n_policy), so that a result never depends on how many images share a call.
static Kernel choose_kernel(const Layer& L, const ConvArgs& a, int precision, int max_batch) {
    const Options& o = options();
    const Kernel tile = L.kernel;
    const long long tiles32 = (long long)((a.Ws + 31) / 32) * max_batch;       // x (tile rows) = workgroups of a 32-wide tile
    if (tile == kFused) return kFused;
    if (L.fused_next >= 0) return kConv1Block;
    if (L.fused_short >= 0) {
        if (L.split)              // IDC_FP16: conv_ds_fused_mh (the bf16 kernel's fp16 twin) where it covers the launch
            return precision == IDC_FP16 && o.fp16_fast && conv_ds_m_applies(a) ? kConvDsM : kConvDsMs;
        return o.ds_m16 && conv_ds_m_applies(a) ? kConvDsM : kConvDs;      // (huge images: conv_ds_fused, 64-bit addressing)
    }
    if (L.spec->kind == kConvIm2col) {
        // conv1_1 with >= 128 big tiles: the 32x32-tile form (the small-tile kernel keeps the batch-1 click path)
        if (L.lprec == IDC_BF16 && a.ksplit <= 1 && tiles32 * ((a.Hs + 31) / 32) >= 128 && conv1_1_bf16_applies(a)) return kConv1_1Bf16;
        // the fp32 island of an operand-split handle where the grid is throughput-sized
        if (is_split(precision) && !L.split && o.conv1_1_split && tiles32 * ((a.Hs + 15) / 16) >= 128 && conv1_1_split_applies(a)) return kConv1_1Split;
    }
    if (L.split) {                // (every operand-split layer is planned on the large tile: set_geometry)
        // IDC_FP16: where the bf16 forward's own kernels cover the launch, their fp16 twins (same tile, bias in the accumulators, packed-pair epilogue)
        if (precision == IDC_FP16 && o.fp16_fast && o.v2p && conv_v2p_applies(L.cfg, L.halo, a)) return kConvV2p;
        if (o.conv1_2_split && conv1_2_split_layer(*L.spec) && tiles32 * ((a.Hs + 11) / 12) >= 256 && conv1_2_split_applies(a)) return kConv1_2Split;
        return o.v2p && conv_v2ps_applies(L.cfg, L.halo, a) ? kConvV2ps : kConvV2s;
    }
    if (tile == kConvV2 && o.mfma16 && conv_v2m_applies(a))      // the 16x16x32-MFMA builds read the layout-1 image
        return o.v2p && conv_v2p_applies(L.cfg, L.halo, a) ? kConvV2p : kConvV2m;
    return tile;
}

// The kernel predicates (conv_*_applies, idc_kernels.h) ask which optional operands a launch carries by testing its pointers.  The plan knows that
// before anything is bound: L's arguments with every pointer bind_layer (idc_exec.hip) will set standing in as a token that is never dereferenced.
static ConvArgs args_as_bound(const Layer& L, const std::vector<Layer>& layers) {
    static const float token = 0.f;
    ConvArgs a = L.args;
    const LayerBlob& bn = L.fused_next >= 0 ? layers[L.fused_next].blob : L.blob;
    auto set = [&](bool carried) -> const float* { return carried ? &token : nullptr; };
    a.in = a.wgt = a.zeros = a.bias = a.head_b = &token;
    a.resid = set(L.fused_short < 0 && L.resid >= 0);
    a.in2 = set(L.fused_short >= 0);
    a.wgt2 = set(L.fused_short >= 0 || L.fused_next >= 0);
    a.bn_scale = set(bn.bn_scale_off != (size_t)-1); a.bn_shift = set(bn.bn_shift_off != (size_t)-1);
    a.img_shift = set(L.shifted);
    a.pk_L = set(L.spec->kind == kConvIm2col);
    a.head_w = set(L.fused_head);
    return a;
}

// The plan of one forward: what every layer launches and with which geometry, as a function of the graph, `env` and options() -- and of nothing
// else: no HIP call, no device pointer, no per-call pointer, no state an earlier forward left in the layers.  run_graph and the single-operator entry
// points (idc_diag.hip) both run it, then bind_layer and launch_kernel per layer.  Every ConvArgs field a launch reads has exactly one writer:
//   fill_taps (once, build_layers)    nphase ntaps so si dy dx tw ro co
//   plan_forward (every forward)      N Hs Ws nkc ncg act tiles_x tiles_y ksplit kc_per (set_geometry; tiles_y = the tile request of a model1 launch)
//                                     out_f32 resid_bf16 nkc2 in_parts out_parts nseg seg_x seg_w w_part_bytes w_part_bytes2 split_f16 warm
//   bind_layer (every launch)         in out wgt bias bn_scale bn_shift resid img_shift in2 wgt2 pk_* head_* acc_scale zeros partial
int plan_forward(std::vector<Layer>& layers, const std::vector<Tensor>& tensors, const PlanEnv& env, std::string* err) {
    const Options& o = options();
    auto geometry = [&](Layer& L, bool allow_v2) {
        const Tensor& sites = tensors[L.spec->kind == kDeconv4x4 ? L.src : L.dst];
        set_geometry(L, L.lprec, env.n, env.max_batch, sites.H, sites.W, allow_v2);
    };
    // the tile family per layer, then which layers ride in another one's launch
    for (auto& L : layers) {
        geometry(L, true);
        L.fused_short = -1; L.fused_next = -1;
        L.shifted = (env.flags & IDC_FLAG_GLOBAL_HINTS) && L.dst == env.t_conv4_3;
    }
    // model1 in one launch: conv1_1 (input pack fused) followed by conv1_2 on the small-tile bf16 path, >= 128 big tiles
    for (size_t i = 0; i + 1 < layers.size(); ++i) {
        Layer& L = layers[i];
        const bool f16blk = env.precision == IDC_FP16 && o.fp16_fast && L.blob.w2_off != (size_t)-1;      // IDC_FP16: conv1_block_fused_th
        if (L.spec->kind != kConvIm2col || (env.precision != IDC_BF16 && !f16blk) || !o.fuse_conv1 || L.spec->act != 1 || L.spec->bnkey) continue;
        // 32x32 tiles when there are >= 128 of them (N = 32); else the 32x8 tile (conv1_block_fused_t<4,2>) when THAT gives >= 128
        // workgroups -- the batch-1 click path: one launch instead of conv1_1 + conv1_2 and no 8 MB intermediate
        const long long t32 = (long long)((env.W + 31) / 32) * ((env.H + 31) / 32) * env.max_batch;
        const long long t8 = (long long)((env.W + 31) / 32) * ((env.H + 7) / 8) * env.max_batch;
        if (t32 < 128 && t8 < 128) continue;
        const int tile_req = t32 >= 128 ? 32 : 8;              // tile height request of launch_conv1_block
        for (size_t j = 0; j < layers.size(); ++j) {
            Layer& P = layers[j];
            const LayerSpec& ps = *P.spec;
            if (P.src != L.dst || (P.kernel == kConvV2 && !f16blk) || ps.kind != kConv3x3 || ps.cin != 64 || ps.cout != 64 || ps.dilation != 1 ||
                ps.in_stride != 1 || ps.act != 1 || ps.resid || tensors[P.dst].is_f32 || P.args.ksplit > 1 || P.kernel == kConvClick ||
                P.kernel == kConvWino) continue;
            bool only_consumer = true;
            for (const Layer& Q : layers) if (&Q != &P && (Q.src == L.dst || Q.resid == L.dst)) only_consumer = false;
            if (only_consumer) { L.fused_next = (int)j; P.kernel = kFused; L.args.tiles_y = tile_req; }
        }
    }
    // a large-tile deconv and the 3x3 shortcut conv it is summed with in one K loop (model.py:156,170,172)
    for (size_t li = 0; li < layers.size(); ++li) {
        Layer& L = layers[li];
        if (L.spec->kind != kDeconv4x4 || L.resid < 0 || L.kernel != kConvV2 || !fuse_shortcut_enabled() || (L.split && !o.split_ds_fuse)) continue;
        if (L.spec->cout % 128 != 0 || L.spec->bnkey || L.spec->act == 2 || tensors[L.dst].is_f32) continue;   // conv_ds_fused's domain
        for (size_t j = 0; j < layers.size(); ++j) {
            Layer& P = layers[j];
            const LayerSpec& ps = *P.spec;
            if (P.dst != L.resid) continue;
            const Tensor& pin = tensors[P.src];
            const Tensor& to = tensors[L.dst];
            // a plain 3x3 conv (no activation, BN or sum of its own) over the deconv's output pixels
            const bool shortcut3x3 = ps.kind == kConv3x3 && ps.dilation == 1 && ps.in_stride == 1 && ps.act == 0 && !ps.bnkey && !ps.resid &&
                                     ps.cout == L.spec->cout && pin.H == to.H && pin.W == to.W && !pin.is_f32;
            if (L.split) {      // operand-split: conv_ds_fused_ms (split tensors in and out, both of the same part count) or two launches
                if (!shortcut3x3 || !P.split || pin.parts != to.parts || tensors[L.src].parts != to.parts || tensors[L.src].is_f32 ||
                    !conv_ds_m_fits(L.args.Hs, L.args.Ws, L.blob.nkc * to.parts, P.blob.nkc * to.parts)) continue;
                // both K loops land in ONE accumulator set with ONE accumulator scale: the packer made the two layers' words equal
                if (env.wscale && li < env.wscale->size() && j < env.wscale->size() && memcmp(&(*env.wscale)[li], &(*env.wscale)[j], 4) != 0)
                    return fail(err, IDC_ERR_INTERNAL, "layers %s and %s would share one launch but their accumulator scales differ (%g, %g): the blob "
                                "was not packed by this library's packer", L.spec->name, ps.name, (double)(*env.wscale)[li], (double)(*env.wscale)[j]);
            } else if (!shortcut3x3 || (kAbPartners ? P.blob.w2_off == (size_t)-1 : !(o.ds_m16 != 0 && conv_ds_m_fits(L.args.Hs, L.args.Ws, L.blob.nkc, P.blob.nkc)))) {
                continue;       // (default library: conv_ds_fused_m or two launches)
            }
            L.fused_short = (int)j; P.kernel = kFused;
        }
    }
    for (auto& L : layers) {
        // the regression head rides in conv10_2's epilogue when one workgroup owns all 128 channels
        L.fused_head = L.dst == env.t_conv10_2 && L.kernel == kConvV2 && L.cfg.wm == 2 && L.args.ncg == 2 && L.spec->bnkey == nullptr;
        // default library: the large tile's 16x16x32 kernels take neither a shortcut SUM (a deconv that was not fused above: images beyond 32-bit
        // offsets) nor a LeakyReLU without the fused head (single operators only) -- the small tile
        if (!kAbPartners && L.kernel == kConvV2 && !L.split && ((L.resid >= 0 && L.fused_short < 0) || (L.spec->act == 2 && !L.fused_head))) {
            geometry(L, false);
            L.fused_head = false;
        }
    }
    // what each launch carries besides pointers, and the entry point it runs
    for (auto& L : layers) {
        if (L.kernel == kFused) continue;
        ConvArgs& a = L.args;
        const Tensor& ti = tensors[L.src];
        const Tensor& to = tensors[L.dst];
        const Layer* S = L.fused_short >= 0 ? &layers[L.fused_short] : nullptr;
        const bool f16_block = L.fused_next >= 0 && env.precision == IDC_FP16;       // conv1_block_fused_th
        const bool island = is_split(env.precision) && !L.split && !f16_block;       // conv_igemm<f32> with a split store
        a.warm = o.code_warm;
        a.split_f16 = split_is_f16(env.precision) ? 1 : 0;
        a.out_f32 = island ? 1 : to.is_f32;
        a.resid_bf16 = (!S && L.resid >= 0 && !tensors[L.resid].is_f32) ? 1 : 0;
        a.nkc2 = S ? S->blob.nkc : 0;
        if (f16_block || island) { a.ksplit = 1; a.kc_per = a.nkc; }                 // (no split-K: its epilogue kernel writes fp32)
        if (island && L.kernel != kConvIgemm) return fail(err, IDC_ERR_INTERNAL, "layer %s: fp32 island outside conv_igemm", L.spec->name);
        // operand-split launch: nseg passes of the K loop (input part x weight part) into one accumulator set; split in / out tensors
        a.in_parts = L.split ? ti.parts : 0;
        a.out_parts = (to.is_f32 || L.fused_head || !(L.split || island)) ? 0 : to.parts;
        a.nseg = L.split ? split_segments(env.precision) : 0;
        a.seg_x = L.split ? split_seg_x(env.precision) : 0u; a.seg_w = L.split ? split_seg_w(env.precision) : 0u;
        a.w_part_bytes = L.split ? L.blob.w_bytes : 0;
        a.w_part_bytes2 = (L.split && S) ? S->blob.w_bytes : 0;
        L.kernel = choose_kernel(L, args_as_bound(L, layers), env.precision, env.max_batch);
        // The small tile is where every layer ends up that no other family covers, and it addresses one source image with 32-bit offsets
        // (conv_igemm_offsets_fit): a layer whose source image is larger has no kernel.  Refused here with the reason -- idc_create asks this
        // plan before it allocates anything -- instead of at the launch.  (conv1_1 reads the caller's planes, not a stored source.)
        if ((L.kernel == kConvIgemm || L.kernel == kConvClick) && L.spec->kind != kConvIm2col && !conv_igemm_offsets_fit(a.Hs, a.Ws, a.si, a.nkc))
            return fail(err, IDC_ERR_INVALID_ARG, "%d x %d is too large for this precision: one image of %s, the source of layer %s, holds %lld bytes; "
                        "the kernel left for that launch (conv_igemm / conv_click) addresses an image of at most 2^31 bytes", env.H, env.W,
                        tensors[L.src].name.c_str(), L.spec->name, (long long)a.Hs * a.si * (long long)a.Ws * a.si * ((long long)a.nkc * kRowBytes));
    }
    return IDC_OK;
}

// What idc_create asks before it touches a device: does every layer of this configuration have a kernel that can address it?  (The plan at
// n = max_batch under the options in force; a later forward plans again and answers the same way.)
int check_geometry(int precision, unsigned flags, int H, int W, int max_batch, std::string* err) {
    const BlobPlan blob = make_blob_plan(precision, flags);
    std::vector<Tensor> tensors;
    std::vector<Layer> layers;
    const int rc = build_layers(blob, precision, H, W, max_batch, tensors, layers, err);
    if (rc) return rc;
    PlanEnv env;
    env.precision = precision; env.flags = flags; env.H = H; env.W = W; env.max_batch = max_batch; env.n = max_batch;
    env.t_conv10_2 = find_tensor(tensors, "conv10_2");
    env.t_conv4_3 = find_tensor(tensors, "conv4_3");
    return plan_forward(layers, tensors, env, err);
}

// One launch of the entry point `k` (kConvKwave: one layer; run_graph tries the persistent chain first).
hipError_t launch_kernel(Kernel k, const Layer& L, const ConvArgs& a, hipStream_t s) {
    switch (k) {
        case kConvIgemm: return launch_conv(L.lprec, L.cfg, L.halo, a, s);
        case kConvClick: return launch_conv_click(L.lprec, L.cfg.wp, L.halo, a, s);
        case kConvWino: return launch_conv_wino(L.lprec, a, s);
        case kDeconvWino: return launch_deconv_wino(L.lprec, a, s);
        case kConvKwave: return launch_conv_kwave(a, s);
        case kConvV2: return launch_conv_v2(L.cfg, L.halo, a, s);
        case kConvV2m: return launch_conv_v2m(L.cfg, L.halo, a, s);
        case kConvV2p: return launch_conv_v2p(L.cfg, L.halo, a, s);
        case kConvV2s: return launch_conv_v2s(L.cfg, L.halo, a, s);
        case kConvV2ps: return launch_conv_v2ps(L.cfg, L.halo, a, s);
        case kConvDs: return launch_conv_ds(a, s);
        case kConvDsM: return launch_conv_ds_m(a, s);
        case kConvDsMs: return launch_conv_ds_ms(a, s);
        case kConv1Block: return launch_conv1_block(a, s);
        case kConv1_1Bf16: return launch_conv1_1_bf16(a, s);
        case kConv1_1Split: return launch_conv1_1_split(a, s);
        case kConv1_2Split: return launch_conv1_2_split(a, s);
        case kFused: break;
    }
    return hipErrorInvalidConfiguration;
}

// The kernel a layer's launch ran (idc_layer_info_get; the names rocprofv3 shows, template arguments as <WM,WP>), from its entry point
void kernel_label(const Layer& L, int precision, char* out, size_t cap) {
    const int wm = L.cfg.wm, wp = L.cfg.wp, nseg = split_segments(precision);
    const bool f16 = split_is_f16(precision), deconv = L.spec->kind == kDeconv4x4;
    const char* const t = L.lprec == IDC_BF16 ? "bf16" : "f32";
    switch (L.kernel) {
        case kConvIgemm: snprintf(out, cap, "conv_igemm<%s,%d,%d>", t, wm, wp); break;
        case kConvClick: snprintf(out, cap, "conv_click<%s,%d,%d>", t, wm, wp); break;
        case kConvWino: snprintf(out, cap, "conv_wino_f32"); break;
        case kDeconvWino: snprintf(out, cap, "conv_wino_deconv_f32"); break;
        case kConvKwave: snprintf(out, cap, deconv ? "conv_kwave_deconv_bf16" : "conv_kwave_bf16"); break;
        case kConvV2: snprintf(out, cap, "conv_igemm_v2<%d,%d>", wm, wp); break;
        case kConvV2m: snprintf(out, cap, "conv_igemm_v2<%d,%d>+m16", wm, wp); break;
        case kConvV2p: snprintf(out, cap, f16 ? "conv_igemm_v2ph<%d,%d>" : "conv_igemm_v2<%d,%d>+m16p", wm, wp); break;
        case kConvV2s: snprintf(out, cap, f16 ? "conv_igemm_v2sh<%d,%d>x%d" : "conv_igemm_v2s<%d,%d>x%d", wm, wp, nseg); break;
        case kConvV2ps: snprintf(out, cap, f16 ? "conv_igemm_v2psh<%d,%d>x%d" : "conv_igemm_v2ps<%d,%d>x%d", wm, wp, nseg); break;
        // (the deconv and its 3x3 shortcut conv in one K loop)
        case kConvDs: snprintf(out, cap, "conv_ds_fused+shortcut"); break;
        case kConvDsM: snprintf(out, cap, f16 ? "conv_ds_fused_mh+shortcut" : "conv_ds_fused_m+shortcut"); break;
        case kConvDsMs: snprintf(out, cap, f16 ? "conv_ds_fused_msh+shortcut x%d" : "conv_ds_fused_ms+shortcut x%d", L.args.nseg); break;
        case kConv1Block: snprintf(out, cap, "conv1_block_fused"); break;
        case kConv1_1Bf16: snprintf(out, cap, "conv1_1_bf16_kernel"); break;
        case kConv1_1Split: snprintf(out, cap, "conv1_1_split_kernel"); break;
        case kConv1_2Split: snprintf(out, cap, "conv1_2_split_kernel x%d", nseg); break;
        case kFused: snprintf(out, cap, "fused"); break;
    }
    if (L.fused_head) strncat(out, "+head", cap - strlen(out) - 1);
    if (L.args.ksplit > 1) {
        char sk[16]; snprintf(sk, sizeof(sk), " splitK%d", L.args.ksplit);
        strncat(out, sk, cap - strlen(out) - 1);
    }
}

static double layer_flops(const LayerSpec& s, int H, int W) {       // per image, SURVEY.md Appendix A
    const double ho = (double)(H / s.level), wo = (double)(W / s.level);
    switch (s.kind) {
        case kConv3x3: case kConvIm2col: return 2.0 * s.cin * s.cout * 9.0 * ho * wo;
        case kConv1x1: return 2.0 * s.cin * s.cout * ho * wo;
        case kDeconv4x4: return 2.0 * s.cin * s.cout * 4.0 * ho * wo;   // 4 taps per OUTPUT pixel
    }
    return 0;
}

// The graph of one configuration: its tensors (shapes and storage; no memory yet) and its layers with their taps.  Needs no device.
int build_layers(const BlobPlan& plan, int precision, int H, int W, int max_batch, std::vector<Tensor>& tensors, std::vector<Layer>& layers, std::string* err) {
    const auto& specs = layer_specs();
    const int eb = elem_bytes(precision);
    const bool split = is_split(precision);
    auto add_tensor = [&](const char* name, int C, int Cpad, int level, int f32) -> int {
        Tensor t;
        t.name = name; t.C = C; t.Cpad = Cpad; t.H = H / level; t.W = W / level; t.is_f32 = f32;
        t.parts = (split && !f32) ? split_parts(precision) : 1;
        t.bytes = (size_t)max_batch * t.H * t.W * Cpad * (f32 ? 4 : eb * t.parts);
        tensors.push_back(t);
        return (int)tensors.size() - 1;
    };
    // operand-split precisions: is tensor `name` read by a layer outside the fp32 island / summed into another layer as a shortcut?
    auto read_by_split_layer = [&](const char* name) {
        for (int ai : plan.active) { const LayerSpec& q = specs[ai]; if (!split_island(q) && strcmp(q.src, name) == 0) return true; }
        return false;
    };
    auto used_as_shortcut = [&](const char* name) {
        for (int ai : plan.active) { const LayerSpec& q = specs[ai]; if (q.resid && strcmp(q.resid, name) == 0) return true; }
        return false;
    };
    tensors[add_tensor("data_l_ab_mask", 36, 64, 1, 0)].bytes = 256;      // never materialised: built inside conv1_1's operand staging
    for (size_t li = 0; li < plan.active.size(); ++li) {
        const LayerSpec& s = specs[plan.active[li]];
        Layer L;
        L.spec = &s; L.blob = plan.layers[li];
        L.src = find_tensor(tensors, s.src);
        if (L.src < 0) return fail(err, IDC_ERR_INVALID_ARG, "graph: unknown source '%s'", s.src);
        if (s.resid) {
            L.resid = find_tensor(tensors, s.resid);
            if (L.resid < 0) return fail(err, IDC_ERR_INVALID_ARG, "graph: unknown residual '%s'", s.resid);
        }
        L.lprec = precision;
        if (split && split_island(s)) {
            // fp32 island (conv1_1): exact-fp32 kernel; its epilogue writes the result as split planes where the split stack reads it
            L.lprec = IDC_FP32;
            L.dst = add_tensor(s.name, s.cout, cout_pad(s.cout), s.level, read_by_split_layer(s.name) ? 0 : 1);
        } else {
            // fp32 storage: everything on the fp32 path; class / 313 logits and the hyper-column partial sums (LayerSpec.out_f32); on the
            // operand-split path also every shortcut branch (summed in fp32 in its consumer's epilogue)
            L.split = split;
            L.dst = add_tensor(s.name, s.cout, cout_pad(s.cout), s.level, precision == IDC_FP32 || s.out_f32 || (split && used_as_shortcut(s.name)));
        }
        fill_taps(L);
        L.flops = layer_flops(s, H, W);
        const Tensor& ti = tensors[L.src];
        const Tensor& to = tensors[L.dst];
        const double in_px = (double)(ti.H / s.in_stride) * (ti.W / s.in_stride);
        L.min_bytes = in_px * ti.Cpad * (ti.is_f32 ? 4 : eb * ti.parts) + (double)to.H * to.W * to.Cpad * (to.is_f32 ? 4 : eb * to.parts) +
                      (L.resid >= 0 ? (double)to.H * to.W * to.Cpad * (tensors[L.resid].is_f32 ? 4 : eb) : 0.0);
        layers.push_back(L);
    }
    return IDC_OK;
}

int build_graph(idc_context* c) {
    const int rc = build_layers(c->plan, c->precision, c->H, c->W, c->max_batch, c->tensors, c->layers, &c->err);
    if (rc) return rc;
    c->t_input = find_tensor(c->tensors, "data_l_ab_mask");
    c->t_conv10_2 = find_tensor(c->tensors, "conv10_2");
    c->t_logits = find_tensor(c->tensors, "class_logits");
    c->t_conv4_3 = find_tensor(c->tensors, "conv4_3");
    c->t_pred313 = find_tensor(c->tensors, "pred_313");
    return IDC_OK;
}

int alloc_graph(idc_context* c) {
    // ONE arena for all activation tensors (3.7 GB at N = 32): a single large allocation is 2 MiB-aligned and physically as
    // contiguous as the driver can make it, whatever the process allocated before -- with one hipMalloc per tensor, a process whose
    // other runtime (torch) had already carved up the address space got some tensors on small pages, and the layers READING those
    // ran 25-35 % slower on every forward (bench.py's conv3_2 / conv5_1 / conv9_2 / conv8_1 against tools/quick_layers.py, which
    // creates the engine first).  IDC_ARENA=0 restores the per-tensor allocations for A/B.
    static const bool use_arena = idc_env_int("IDC_ARENA", 1) != 0;
    if (use_arena) {
        const size_t al = (size_t)2 << 20;
        size_t total = 0;
        for (auto& t : c->tensors) total += align_up(t.bytes, al);
        HIPCHK(c, c->d_arena.ensure(total));
        size_t off = 0;
        for (auto& t : c->tensors) { t.ptr = (char*)c->d_arena.get() + off; off += align_up(t.bytes, al); }
    } else {
        c->tensor_mem.resize(c->tensors.size());
        for (size_t i = 0; i < c->tensors.size(); ++i) {
            HIPCHK(c, c->tensor_mem[i].ensure(c->tensors[i].bytes));
            c->tensors[i].ptr = c->tensor_mem[i].get();
        }
    }
    const size_t hw = (size_t)c->H * c->W, nb = (size_t)c->max_batch;
    HIPCHK(c, c->d_L.ensure(nb * hw * 4));
    HIPCHK(c, c->d_ab.ensure(nb * hw * 2 * 4));
    HIPCHK(c, c->d_mask.ensure(nb * hw * 4));
    HIPCHK(c, c->d_out.ensure(nb * hw * 2 * 4));
    // resident planes start defined: no hints (ab = 0, mask = 0); an L plane has to be uploaded before a resident forward
    HIPCHK(c, hipMemset(c->d_L.get(), 0, nb * hw * 4));
    HIPCHK(c, hipMemset(c->d_ab.get(), 0, nb * hw * 2 * 4));
    HIPCHK(c, hipMemset(c->d_mask.get(), 0, nb * hw * 4));
    HIPCHK(c, hipMemset(c->d_out.get(), 0, nb * hw * 2 * 4));
    c->l_set.assign(nb, 0);
    c->src.resize(nb);
    c->hint_mask_value.assign(nb, 0.f);
    HIPCHK(c, c->d_zeros.ensure(256));
    HIPCHK(c, hipMemset(c->d_zeros.get(), 0, 256));
    if (c->precision == IDC_BF16) {              // conv_kwave_chain_bf16's grid-barrier counter and its host-visible abort flag
        HIPCHK(c, c->d_kw_bar.ensure(1024));
        HIPCHK(c, hipMemset(c->d_kw_bar.get(), 0, 1024));
        HIPCHK(c, c->h_kw_abort.ensure(64));
        *c->h_kw_abort.get() = 0;
    }
    // the memsets above run on the NULL stream, the kernels on the handle's non-blocking stream: every conv launch reads the
    // zero page (out-of-image halo rows), so make the fills complete before the handle can launch anything
    HIPCHK(c, hipStreamSynchronize(nullptr));
    HIPCHK(c, c->ev_sync.create(hipEventDisableTiming));
    HIPCHK(c, c->h_in.ensure(nb * hw * 4 * 4));
    HIPCHK(c, c->h_out.ensure(nb * hw * 2 * 4));
    if (c->flags & IDC_FLAG_DIST_HEAD) {
        const size_t dq = nb * 529 * (hw / 16) * 4;
        HIPCHK(c, c->d_dist.ensure(dq));
        HIPCHK(c, c->h_dist.ensure(dq));
    }
    if (c->flags & IDC_FLAG_DIST313) {
        HIPCHK(c, c->d_pred_ab.ensure(nb * hw * 2 * 4));
        HIPCHK(c, c->h_pred_ab.ensure(nb * hw * 2 * 4));
        HIPCHK(c, c->d_dist313.ensure(nb * hw * 313 * 4));      // 82 MB per 256x256 image: sized for 288 GB parts
    }
    if (c->flags & IDC_FLAG_GLOBAL_HINTS) {
        HIPCHK(c, c->d_glob_in.ensure(nb * kGlobIn * 4));
        HIPCHK(c, c->d_glob_vec.ensure(nb * kGlobC * 4));
        HIPCHK(c, hipMemset(c->d_glob_in.get(), 0, nb * kGlobIn * 4));
    }
    c->n_timed = (int)c->layers.size() + 3;           // profiling events (2240 per handle) are created by idc_set_profiling, not here:
    return IDC_OK;                                    // a process holding many handles must not exhaust the runtime's signal pool
}

}  // namespace idc

extern "C" {

int idc_set_splitk_policy(int policy) {
    if (policy < 0 || policy > 2) return fail(nullptr, IDC_ERR_INVALID_ARG, "split-K policy %d not in 0..2", policy);
    options().splitk_policy = policy;
    return IDC_OK;
}

int idc_set_tile_policy(int policy) {
    if (policy < 0 || policy > 2) return fail(nullptr, IDC_ERR_INVALID_ARG, "tile policy %d not in 0..2", policy);
    options().tile_policy = policy;
    return IDC_OK;
}

int idc_set_option(const char* name, int value) {
    Options& o = options();
    if (!name) return fail(nullptr, IDC_ERR_INVALID_ARG, "null option name");
    if (strcmp(name, "fuse_conv1") == 0) { o.fuse_conv1 = value != 0; return IDC_OK; }
    if (strcmp(name, "click") == 0) { o.click = value; return IDC_OK; }
    if (strcmp(name, "winograd") == 0) {         // 0 off | 1 automatic | 2 everywhere implemented | 12 / 21 / 22 automatic, 3x3 form <TB,CB> forced
        if (value != 0 && value != 1 && value != 2 && value != 12 && value != 21 && value != 22)
            return fail(nullptr, IDC_ERR_INVALID_ARG, "option 'winograd': %d not in {0, 1, 2, 12, 21, 22}", value);
        o.wino = value != 0;
        o.wino_deconv = value == 2 ? 2 : 1;
        set_wino_form(value >= 12 ? value : 0);
        return IDC_OK;
    }
    if (!kAbPartners && ((strcmp(name, "mfma16") == 0 && value == 0) || (strcmp(name, "ds_mfma16") == 0 && value == 0)))
        return fail(nullptr, IDC_ERR_UNSUPPORTED, "option '%s' = 0 selects a 32x32x16-MFMA partner kernel: not in the default library (build with make EXTRA=-DIDC_AB_PARTNERS)", name);
    if (strcmp(name, "mfma16") == 0) { o.mfma16 = value != 0; return IDC_OK; }
    if (strcmp(name, "v2p") == 0) { o.v2p = value != 0; return IDC_OK; }
    if (strcmp(name, "ds_mfma16") == 0) { o.ds_m16 = value != 0; set_ds_half(value != 2); return IDC_OK; }     // 2: conv_ds_fused_m, 8-wave workgroups on every grid
    if (strcmp(name, "split_ds_fuse") == 0) { o.split_ds_fuse = value != 0; return IDC_OK; }
    if (strcmp(name, "conv1_1_split") == 0) { o.conv1_1_split = value != 0; return IDC_OK; }
    if (strcmp(name, "conv1_2_split") == 0) { o.conv1_2_split = value != 0; return IDC_OK; }
    if (strcmp(name, "fp16_fast") == 0) { o.fp16_fast = value != 0; return IDC_OK; }
    if (strcmp(name, "kwave") == 0) { o.kwave = value != 0; return IDC_OK; }
    if (strcmp(name, "spin_sync") == 0) { o.spin_sync = value != 0; return IDC_OK; }
    if (strcmp(name, "pcie_kernel") == 0) { o.pcie_kernel = value != 0; return IDC_OK; }
    if (strcmp(name, "kw_force_abort") == 0) { o.kw_force_abort = value != 0; return IDC_OK; }
    if (strcmp(name, "grid_cap") == 0) {         // test hook: idc_grid.h
        if (value < 0) return fail(nullptr, IDC_ERR_INVALID_ARG, "option 'grid_cap': %d is negative", value);
        set_grid_cap(value);
        return IDC_OK;
    }
    if (strcmp(name, "op_policy_batch") == 0) {
        if (value < 0) return fail(nullptr, IDC_ERR_INVALID_ARG, "option 'op_policy_batch': %d is negative", value);
        o.op_policy_batch = value;
        return IDC_OK;
    }
    if (strcmp(name, "op_out_f32") == 0) { o.op_out_f32 = value != 0; return IDC_OK; }
    if (strcmp(name, "op_resid_f32") == 0) { o.op_resid_f32 = value != 0; return IDC_OK; }
    if (strcmp(name, "kwave_chain") == 0) { o.kwave_chain = value < 0 ? 0 : (value > 2 ? 2 : value); return IDC_OK; }
    return fail(nullptr, IDC_ERR_INVALID_ARG, "unknown option '%s'", name);
}

}  // extern "C"
