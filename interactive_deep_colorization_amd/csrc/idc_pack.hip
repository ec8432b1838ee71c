// idc_pack.hip -- the weight blob: its plan (make_blob_plan), the packer that turns a state_dict into the MFMA-tiled, swizzled images the kernels
// read, and the weight part of the C ABI (include/ideepcolor.h): pack, validate, load, set.
// Replaces: the load_state_dict/eval part of ColorizeImageTorch.prep_net (data/colorize_image.py:216-233).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "idc_engine.h"

namespace idc {

BlobPlan make_blob_plan(int precision, unsigned flags) {
    BlobPlan p;
    p.precision = precision;
    p.flags = flags & (IDC_FLAG_DIST_HEAD | IDC_FLAG_GLOBAL_HINTS | IDC_FLAG_DIST313 | IDC_FLAG_THROUGHPUT_BLOB);
    // Winograd U images: the fp32 path only (round 5: the bf16 click path's Winograd kernels were retired -- conv_kwave_* read the layout-1
    // images -- so a bf16 blob is 70 MB (136 MB with the partner build's layout-2 images) whatever the flag says; fp32: 384 MB, 136 MB with
    // IDC_FLAG_THROUGHPUT_BLOB)
    const bool wino_images = !(flags & IDC_FLAG_THROUGHPUT_BLOB) && precision == IDC_FP32;
    const auto& specs = layer_specs();
    size_t off = sizeof(BlobHeader);
    for (int i = 0; i < (int)specs.size(); ++i) {
        const LayerSpec& s = specs[i];
        if (s.dist_only == 1 && !(flags & IDC_FLAG_DIST_HEAD)) continue;
        if (s.dist_only == 2 && !(flags & IDC_FLAG_DIST313)) continue;
        LayerBlob lb;
        // operand-split precisions: model1 is an fp32 island (fp32 images incl. conv1_2's Winograd image), every other layer carries
        // split_parts() layout-1 bf16 images
        lb.f32 = is_split(precision) && split_island(s);
        lb.parts = (is_split(precision) && !lb.f32) ? split_parts(precision) : 1;
        const int lprec = lb.f32 ? (int)IDC_FP32 : precision;
        const int kc = kc_elems(lprec);
        const bool wino_l = lb.f32 ? true : wino_images;
        const int kch = k_channels(s);
        lb.nkc = (s.kind == kConvIm2col) ? (64 / kc) : (kch + kc - 1) / kc;   // conv1_1 operand is 64 wide
        lb.ncg = cout_pad(s.cout) / kCoutGroup;
        lb.w_bytes = (size_t)weight_taps(s.kind) * lb.nkc * lb.ncg * kWBlockBytes;
        off = align_up(off, 256); lb.w_off = off; off += lb.w_bytes * lb.parts;
        lb.w2_off = (size_t)-1;
        // (layout 2 = the 32x32x16-MFMA kernels' image: partner build only; the default library's bf16 blob is 70 MB instead of 136)
        if (kAbPartners && precision == IDC_BF16 && v2_eligible(s)) { off = align_up(off, 256); lb.w2_off = off; off += lb.w_bytes; }
        // IDC_FP16: conv1_1 also as ONE fp16 layout-1 block (K = 36 in a 64-wide chunk) -- what conv1_block_fused_th reads; the fp32 island image above stays
        // for the launches the block does not take
        if (precision == IDC_FP16 && s.kind == kConvIm2col) { off = align_up(off, 256); lb.w2_off = off; off += kWBlockBytes; }
        lb.w3_off = (size_t)-1; lb.w3_bytes = 0;
        if (wino_l && wino_eligible(s) && s.cin % kc == 0) {                            // fp32: every batch size; bf16: the batch-1 click path
            lb.w3_bytes = (size_t)s.cin * cout_pad(s.cout) * 16 * elem_bytes(lprec);   // 16 transformed values per (cin, cout)
            off = align_up(off, 256); lb.w3_off = off; off += lb.w3_bytes;
        }
        if (wino_l && wino_deconv_eligible(s) && s.cin % kc == 0) {                      // deconvs: F(2x2,2x2) over the four phases (click path)
            lb.w3_bytes = (size_t)s.cin * cout_pad(s.cout) * 36 * elem_bytes(lprec);
            off = align_up(off, 256); lb.w3_off = off; off += lb.w3_bytes;
        }
        off = align_up(off, 256); lb.bias_off = off; off += (size_t)cout_pad(s.cout) * 4;
        if (s.bnkey) {
            off = align_up(off, 256); lb.bn_scale_off = off; off += (size_t)cout_pad(s.cout) * 4;
            off = align_up(off, 256); lb.bn_shift_off = off; off += (size_t)cout_pad(s.cout) * 4;
        } else {
            lb.bn_scale_off = lb.bn_shift_off = (size_t)-1;
        }
        lb.fbias_off = (size_t)-1;
        if (s.resid) { off = align_up(off, 256); lb.fbias_off = off; off += (size_t)cout_pad(s.cout) * 4; }
        if (is_split(precision) && !lb.f32) { off = align_up(off, 256); lb.wscale_off = off; off += 4; }     // 2^-s of weights packed as w * 2^s (IDC_FP16X3; else 1.0)
        p.layers.push_back(lb);
        p.active.push_back(i);
    }
    off = align_up(off, 256); p.head_w_off = off; off += 2 * 128 * 4;
    off = align_up(off, 256); p.head_b_off = off; off += 2 * 4;
    p.pred_ab_off = (size_t)-1;
    if (flags & IDC_FLAG_DIST313) { off = align_up(off, 256); p.pred_ab_off = off; off += (2 * 313 + 2) * 4; }
    p.glob_off = (size_t)-1;
    if (flags & IDC_FLAG_GLOBAL_HINTS) { off = align_up(off, 256); p.glob_off = off; off += glob_param_floats() * 4; }
    p.total_bytes = align_up(off, 256);
    return p;
}

static uint64_t fnv1a(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

struct TensorView {
    const float* data = nullptr;
    int ndim = 0;
    int64_t dims[4] = {0, 0, 0, 0};
};

static bool dims_are(const TensorView& t, std::initializer_list<int64_t> d) {
    if (t.ndim != (int)d.size()) return false;
    int i = 0;
    for (int64_t v : d) if (t.dims[i++] != v) return false;
    return true;
}

// Write one element of the packed weight image (layout 1: small-tile kernels, layout 2: conv_igemm_v2).
// part: operand-split precisions -- which part of the weight is stored (0 = hi: rne(v); 1: rne(v - hi); 2: rne(v - hi - mid))
static inline void put_w(uint8_t* wimg, int precision, int layout, int nkc, int ncg, int tw, int co, int k, float v, int part, float wmul = 1.f) {
    v *= wmul;                                                     // (a power of two: exact)
    const int kc_e = kc_elems(precision), eb = elem_bytes(precision), eps = kSlotBytes / eb;
    const int kc = k / kc_e, kin = k % kc_e;
    const int s = kin / eps, e = kin % eps;
    const int cg = co / kCoutGroup, col = co % kCoutGroup;
    int lam, sig;
    if (layout == 2) {
        lam = cg_cout_to_row2(col);
        sig = s ^ swz2(lam);
    } else {
        // inverse of cg_row_to_cout: col = g*16 + ci*4 + reg  ->  lam = ci*16 + g*4 + reg
        const int gq = col >> 4, ci = (col >> 2) & 3, reg = col & 3;
        lam = ci * 16 + gq * 4 + reg;
        sig = s ^ swz(lam);
    }
    const size_t off = ((size_t)(tw * nkc + kc) * ncg + cg) * kWBlockBytes + (size_t)lam * kRowBytes +
                       (size_t)sig * kSlotBytes + (size_t)e * eb;
    if (split_is_f16(precision)) {                                 // IDC_FP16X3: fp16 parts (RNE; weights beyond the fp16 range saturate)
        auto to_h = [](float x) { return (_Float16)(x > 65504.f ? 65504.f : (x < -65504.f ? -65504.f : x)); };
        _Float16 b = to_h(v);
        for (int q = 0; q < part; ++q) { v -= (float)b; b = to_h(v); }
        memcpy(wimg + off, &b, 2);
    } else if (precision != IDC_FP32) {
        uint16_t b = f32_to_bf16_rne(v);
        for (int q = 0; q < part; ++q) {                           // (exact: the remainder of a round-to-nearest is representable)
            uint32_t u = (uint32_t)b << 16; float hi; memcpy(&hi, &u, 4);
            v -= hi;
            b = f32_to_bf16_rne(v);
        }
        memcpy(wimg + off, &b, 2);
    } else {
        memcpy(wimg + off, &v, 4);
    }
}

// Pack one conv-like layer: weights in torch layout -> MFMA-tiled, swizzled image.
// IDC_FP16X3: the power of two s that brings max|w| into [8192, 16384) -- hi = rne16(w 2^s) uses fp16's top binades, lo = rne16(w 2^s - hi) is a NORMAL fp16
// number down to weights 2^-17 of the largest; unscaled, he-style weights (~0.02) have lo parts ~1e-5, below fp16's smallest normal 6.1e-5, and keep only
// 6e-8 absolute = 2^-18 of the weight (measured, oracle/emulate.py + tools/split_study.py: N = 1 he-style 2.7e-3 -> 9.5e-4 on the ab map, fp32 arithmetic 1.2e-3)
int f16_weight_exponent(const float* w, size_t n) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) { const float a = fabsf(w[i]); if (a > mx && a < INFINITY) mx = a; }
    if (mx == 0.f) return 0;
    int e; (void)frexpf(mx, &e);                                   // mx = m 2^e, m in [0.5, 1)
    int s = 14 - e;                                                // mx 2^s in [8192, 16384)
    return s < -10 ? -10 : (s > 40 ? 40 : s);
}

void pack_layer_weights(uint8_t* wimg, int precision, int layout, const LayerSpec& s, const LayerBlob& lb,
                               const float* w, int part, float wmul) {
    memset(wimg, 0, lb.w_bytes);
    const int cin = s.cin, cout = s.cout;
    if (s.kind == kConv3x3) {
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < 9; ++t)
                    put_w(wimg, precision, layout, lb.nkc, lb.ncg, t, co, ci, w[((size_t)co * cin + ci) * 9 + t], part, wmul);
    } else if (s.kind == kConvIm2col) {          // K index = tap*4 + c  (the order conv1_1's fused input pack builds)
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < 9; ++t)
                    put_w(wimg, precision, layout, lb.nkc, lb.ncg, 0, co, t * 4 + ci, w[((size_t)co * cin + ci) * 9 + t], part, wmul);
    } else if (s.kind == kConv1x1) {
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci)
                put_w(wimg, precision, layout, lb.nkc, lb.ncg, 0, co, ci, w[(size_t)co * cin + ci], part, wmul);
    } else {                                      // ConvTranspose2d weight is (Cin, Cout, 4, 4)
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < cout; ++co)
                for (int t = 0; t < 16; ++t)
                    put_w(wimg, precision, layout, lb.nkc, lb.ncg, t, co, ci, w[((size_t)ci * cout + co) * 16 + t], part, wmul);
    }
}

// Winograd F(2x2,3x3) weight image of one 3x3 layer (fp32 path, idc_wino.hip): U = G g G^T per (cout, cin) in float64,
// G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], stored in MFMA A-operand order
//   [chunk = ci/32][pos = i*4+j][cout block = co/16][ks][lane = g*16 + co%16][e],   ci%32 = (ks*4 + g)*4 + e
// so that one wave-wide 16-byte load is the fragment of (pos, 16 couts, 16 cin).
// bf16: chunk = ci/64, ci%64 = (ks*4 + g)*8 + e, 8 bf16 per lane; U rounded to bf16 once, from the float64 transform.
void pack_wino_weights(uint8_t* img, int precision, const LayerSpec& s, const LayerBlob& lb, const float* w) {
    memset(img, 0, lb.w3_bytes);
    static const double G[4][3] = {{1, 0, 0}, {.5, .5, .5}, {.5, -.5, .5}, {0, 0, 1}};
    const int ncb = cout_pad(s.cout) / 16;
    const int kc = kc_elems(precision), eps = kSlotBytes / elem_bytes(precision);     // channels per chunk, elements per 16-byte slot
    float* const out = (float*)img;
    uint16_t* const out16 = (uint16_t*)img;
    for (int co = 0; co < s.cout; ++co)
        for (int ci = 0; ci < s.cin; ++ci) {
            const float* g = w + ((size_t)co * s.cin + ci) * 9;
            double t[4][3];
            for (int i = 0; i < 4; ++i)
                for (int kx = 0; kx < 3; ++kx) t[i][kx] = G[i][0] * g[0 * 3 + kx] + G[i][1] * g[1 * 3 + kx] + G[i][2] * g[2 * 3 + kx];
            const int c = ci / kc, within = ci % kc, slot = within / eps, e = within % eps, ks = slot / 4, gq = slot % 4;
            const int cbg = co / 16, m = co % 16, lane = gq * 16 + m;
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    const double u = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];
                    const size_t idx = (((((size_t)c * 16 + (i * 4 + j)) * ncb + cbg) * 2 + ks) * 64 + lane) * eps + e;
                    if (precision == IDC_BF16) out16[idx] = f32_to_bf16_rne((float)u);
                    else out[idx] = (float)u;
                }
        }
}

// Winograd F(2x2,2x2) image of a ConvTranspose 4x4 s2 p1 layer (fp32, conv_wino_deconv_f32): per output phase (r,s) the 2x2 sub-kernel
// g[a][b] = W[ci][co][KY[r][a]][KY[s][b]], KY = {{3,1},{2,0}} (taps in ascending input offset: SURVEY.md Appendix C), U = G g G^T
// with G = [[1,0],[1,1],[0,1]]; position p = ((r*2+s)*3 + i)*3 + j; same fragment order as pack_wino_weights with 36 positions.
void pack_wino_deconv_weights(uint8_t* img, int precision, const LayerSpec& s, const LayerBlob& lb, const float* w) {
    memset(img, 0, lb.w3_bytes);
    static const int KY[2][2] = {{3, 1}, {2, 0}};
    const int ncb = cout_pad(s.cout) / 16;
    const int kc = kc_elems(precision), eps = kSlotBytes / elem_bytes(precision);
    float* const out = (float*)img;
    uint16_t* const out16 = (uint16_t*)img;
    for (int ci = 0; ci < s.cin; ++ci)
        for (int co = 0; co < s.cout; ++co) {
            const float* g16 = w + ((size_t)ci * s.cout + co) * 16;             // (Cin, Cout, 4, 4)
            const int c = ci / kc, within = ci % kc, slot = within / eps, e = within % eps, ks = slot / 4, gq = slot % 4;
            const int cbg = co / 16, m = co % 16, lane = gq * 16 + m;
            for (int r = 0; r < 2; ++r)
                for (int sx = 0; sx < 2; ++sx) {
                    double g[2][2];
                    for (int a = 0; a < 2; ++a)
                        for (int b = 0; b < 2; ++b) g[a][b] = g16[KY[r][a] * 4 + KY[sx][b]];
                    const double t[3][2] = {{g[0][0], g[0][1]}, {g[0][0] + g[1][0], g[0][1] + g[1][1]}, {g[1][0], g[1][1]}};   // G g
                    for (int i = 0; i < 3; ++i) {
                        const double u3[3] = {t[i][0], t[i][0] + t[i][1], t[i][1]};                                       // (G g) G^T
                        for (int j = 0; j < 3; ++j) {
                            const int p = ((r * 2 + sx) * 3 + i) * 3 + j;
                            const size_t idx = (((((size_t)c * 36 + p) * ncb + cbg) * 2 + ks) * 64 + lane) * eps + e;
                            if (precision == IDC_BF16) out16[idx] = f32_to_bf16_rne((float)u3[j]);
                            else out[idx] = (float)u3[j];
                        }
                    }
                }
        }
}

// the queued image packers on up to 16 host threads (each writes its own image: no sharing)
static void run_pack_tasks(std::vector<std::function<void()>>& t) {
    if (t.empty()) return;
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 4 : (nt > 16 ? 16 : nt);
    if (nt > t.size()) nt = (unsigned)t.size();
    std::atomic<size_t> next{0};
    auto work = [&]() { for (size_t i; (i = next.fetch_add(1)) < t.size();) t[i](); };
    std::vector<std::thread> th;
    for (unsigned k = 1; k < nt; ++k) th.emplace_back(work);
    work();
    for (auto& x : th) x.join();
    t.clear();
}

// Activation exponents (idc_pack_weights_ex): what the caller asked for, resolved into what the graph can carry.  a_out[li]: active layer li's output is
// stored as value * 2^a_out; a_in[li]: the exponent of the tensor it reads.  Forced to 0: the fp32 island, fp32 outputs and conv10_2 (the head reads it
// unscaled in its own epilogue).  A shortcut conv takes the exponent of the ConvTranspose it is summed into (fused: one accumulator set; unfused: its fp32
// sums join the deconv's accumulators before the activation).
static int resolve_act_exp(const BlobPlan& plan, int precision, unsigned flags, const int* act_exp, int n_layers, std::vector<int>* a_out,
                           std::vector<int>* a_in, std::string* err) {
    const auto& specs = layer_specs();
    const size_t nl = plan.active.size();
    a_out->assign(nl, 0); a_in->assign(nl, 0);
    if (!act_exp) return IDC_OK;
    if (n_layers != (int)nl + 3)
        return fail(err, IDC_ERR_INVALID_ARG, "act_exp: n_layers %d, but the layer table of these flags has %d rows", n_layers, (int)nl + 3);
    bool any = false;
    for (size_t li = 0; li < nl; ++li) {
        const int a = act_exp[li + 1];
        if (a < -kActExpMax || a > kActExpMax) return fail(err, IDC_ERR_INVALID_ARG, "act_exp[%d] = %d outside +-%d", (int)li + 1, a, kActExpMax);
        any = any || a != 0;
    }
    if (!any) return IDC_OK;
    if (precision != IDC_FP16X3)
        return fail(err, IDC_ERR_UNSUPPORTED, "non-zero activation exponents need precision IDC_FP16X3 (got %d): the other precisions carry no accumulator scale", precision);
    if (flags & (IDC_FLAG_DIST_HEAD | IDC_FLAG_DIST313 | IDC_FLAG_GLOBAL_HINTS))
        return fail(err, IDC_ERR_UNSUPPORTED, "non-zero activation exponents are not supported with %s: it reads or adds to tensors that would be scaled",
                    (flags & IDC_FLAG_DIST_HEAD) ? "IDC_FLAG_DIST_HEAD" : (flags & IDC_FLAG_DIST313) ? "IDC_FLAG_DIST313" : "IDC_FLAG_GLOBAL_HINTS");
    if (nl > sizeof(((BlobHeader*)nullptr)->pad)) return fail(err, IDC_ERR_INTERNAL, "act_exp: %d layers do not fit the blob header", (int)nl);
    auto find = [&](const char* name) { for (size_t lj = 0; lj < nl; ++lj) if (strcmp(specs[plan.active[lj]].name, name) == 0) return (int)lj; return -1; };
    for (size_t li = 0; li < nl; ++li) {
        const LayerSpec& s = specs[plan.active[li]];
        (*a_out)[li] = (plan.layers[li].f32 || s.out_f32 || strcmp(s.name, "conv10_2") == 0) ? 0 : act_exp[li + 1];
    }
    for (size_t li = 0; li < nl; ++li) {
        const LayerSpec& s = specs[plan.active[li]];
        const int lj = s.resid ? find(s.resid) : -1;
        if (lj >= 0) (*a_out)[lj] = (*a_out)[li];
    }
    for (size_t li = 0; li < nl; ++li) {
        const int lj = find(specs[plan.active[li]].src);
        (*a_in)[li] = lj >= 0 ? (*a_out)[lj] : 0;
    }
    return IDC_OK;
}

static int pack_weights_impl(int precision, unsigned flags, const idc_tensor_desc* tensors, int n_tensors,
                             void* blob, size_t blob_bytes, std::string* err, const int* act_exp = nullptr, int n_layers = 0) {
    if (precision < IDC_FP32 || precision > IDC_FP16) return fail(err, IDC_ERR_INVALID_ARG, "bad precision %d", precision);
    if (!tensors || n_tensors <= 0 || !blob) return fail(err, IDC_ERR_INVALID_ARG, "null tensors/blob");
    const BlobPlan plan = make_blob_plan(precision, flags);
    std::vector<int> a_out, a_in;
    {
        const int arc = resolve_act_exp(plan, precision, flags, act_exp, n_layers, &a_out, &a_in, err);
        if (arc) return arc;
    }
    if (blob_bytes < plan.total_bytes)
        return fail(err, IDC_ERR_INVALID_ARG, "blob too small: %zu < %zu", blob_bytes, plan.total_bytes);
    std::map<std::string, TensorView> sd;
    for (int i = 0; i < n_tensors; ++i) {
        if (!tensors[i].name || !tensors[i].data) return fail(err, IDC_ERR_INVALID_ARG, "tensor %d has null name/data", i);
        TensorView v;
        v.data = tensors[i].data;
        v.ndim = tensors[i].ndim;
        for (int d = 0; d < 4 && d < v.ndim; ++d) v.dims[d] = tensors[i].dims[d];
        sd[tensors[i].name] = v;
    }
    auto need = [&](const std::string& key, const TensorView** out) -> bool {
        auto it = sd.find(key);
        if (it == sd.end()) return false;
        *out = &it->second;
        return true;
    };
    uint8_t* const base = (uint8_t*)blob;
    memset(base, 0, plan.total_bytes);
    const auto& specs = layer_specs();
    std::vector<std::function<void()>> tasks;
    // IDC_FP16X3: per-layer power-of-two weight scale (f16_weight_exponent); a deconv and the shortcut conv it is summed with share ONE (the smaller
    // exponent): conv_ds_fused_ms accumulates both K loops into one accumulator set.  Every other precision: exponent 0.
    std::vector<int> wexp(plan.active.size(), 0);
    if (split_is_f16(precision) && split_parts(precision) > 1) {       // (IDC_FP16, one part: a weight keeps its 11 bits down to 6e-5 unscaled)
        for (size_t li = 0; li < plan.active.size(); ++li) {
            const LayerSpec& s = specs[plan.active[li]];
            if (plan.layers[li].f32) continue;
            const TensorView* w = nullptr;
            if (!need(std::string(s.wkey) + ".weight", &w)) continue;      // (reported by the loop below)
            size_t cnt = 1;
            for (int d = 0; d < w->ndim; ++d) cnt *= (size_t)w->dims[d];
            wexp[li] = f16_weight_exponent(w->data, cnt);
        }
        for (size_t li = 0; li < plan.active.size(); ++li) {
            const LayerSpec& s = specs[plan.active[li]];
            if (!s.resid) continue;
            for (size_t lj = 0; lj < plan.active.size(); ++lj)
                if (strcmp(specs[plan.active[lj]].name, s.resid) == 0 && !plan.layers[lj].f32 && !plan.layers[li].f32) {
                    // ONE accumulator scale 2^-(wexp + a_in) for both K loops: the larger side's weight exponent comes down (a_in = 0: the smaller wexp for both)
                    const int t = std::min(wexp[li] + a_in[li], wexp[lj] + a_in[lj]);
                    wexp[li] = t - a_in[li]; wexp[lj] = t - a_in[lj];
                }
        }
    }
    for (size_t li = 0; li < plan.active.size(); ++li) {
        const LayerSpec& s = specs[plan.active[li]];
        const LayerBlob& lb = plan.layers[li];
        const TensorView *w = nullptr, *b = nullptr;
        const std::string wk = std::string(s.wkey) + ".weight", bk = std::string(s.wkey) + ".bias";
        if (!need(wk, &w)) return fail(err, IDC_ERR_MISSING_KEY, "missing state_dict key '%s'", wk.c_str());
        if (!need(bk, &b)) return fail(err, IDC_ERR_MISSING_KEY, "missing state_dict key '%s'", bk.c_str());
        bool ok;
        if (s.kind == kDeconv4x4) ok = dims_are(*w, {s.cin, s.cout, 4, 4});
        else if (s.kind == kConv1x1) ok = dims_are(*w, {s.cout, s.cin, 1, 1});
        else ok = dims_are(*w, {s.cout, s.cin, 3, 3});
        if (!ok) return fail(err, IDC_ERR_MISSING_KEY, "key '%s' has the wrong shape", wk.c_str());
        if (!dims_are(*b, {s.cout})) return fail(err, IDC_ERR_MISSING_KEY, "key '%s' has the wrong shape", bk.c_str());
        const int lprec = lb.f32 ? (int)IDC_FP32 : precision;        // (operand-split precisions: model1's fp32 island)
        // the weight images are independent of each other: queued here, packed by the worker threads below (round 6: 1.4 s -> 0.2 s for a bf16 blob)
        const LayerSpec* sp = &s; const LayerBlob* lbp = &lb; const float* wd = w->data;
        const float wmul = ldexpf(1.f, wexp[li]);
        // the accumulators come back from weights * 2^wexp and inputs * 2^a_in; a layer without BatchNorm also puts its own output exponent here and on its
        // bias (act(x) 2^a = act(x 2^a): ReLU / LeakyReLU / none are positively homogeneous), a layer with one on the BatchNorm scale and shift below
        const int a_epi = s.bnkey ? 0 : a_out[li];
        if (lb.wscale_off != (size_t)-1) *(float*)(base + lb.wscale_off) = ldexpf(1.f, a_epi - wexp[li] - a_in[li]);
        for (int part = 0; part < lb.parts; ++part)
            tasks.push_back([=]() { pack_layer_weights(base + lbp->w_off + (size_t)part * lbp->w_bytes, lprec, 1, *sp, *lbp, wd, part, wmul); });
        if (precision == IDC_FP16 && s.kind == kConvIm2col && lb.w2_off != (size_t)-1) {
            LayerBlob lbc = lb; lbc.nkc = 1; lbc.w_bytes = kWBlockBytes;           // one 64-wide fp16 chunk
            tasks.push_back([=]() { pack_layer_weights(base + lbc.w2_off, (int)IDC_FP16, 1, *sp, lbc, wd, 0, 1.f); });
        } else if (lb.w2_off != (size_t)-1) tasks.push_back([=]() { pack_layer_weights(base + lbp->w2_off, lprec, 2, *sp, *lbp, wd); });
        if (lb.w3_off != (size_t)-1) {
            if (s.kind == kDeconv4x4) tasks.push_back([=]() { pack_wino_deconv_weights(base + lbp->w3_off, lprec, *sp, *lbp, wd); });
            else tasks.push_back([=]() { pack_wino_weights(base + lbp->w3_off, lprec, *sp, *lbp, wd); });
        }
        float* bias = (float*)(base + lb.bias_off);
        for (int c = 0; c < s.cout; ++c) bias[c] = a_epi ? ldexpf(b->data[c], a_epi) : b->data[c];
        if (s.bnkey) {
            const TensorView *g = nullptr, *be = nullptr, *mu = nullptr, *var = nullptr;
            const std::string p = s.bnkey;
            if (!need(p + ".weight", &g) || !need(p + ".bias", &be) || !need(p + ".running_mean", &mu) ||
                !need(p + ".running_var", &var))
                return fail(err, IDC_ERR_MISSING_KEY, "missing BatchNorm keys under '%s'", s.bnkey);
            if (!dims_are(*g, {s.cout}) || !dims_are(*be, {s.cout}) || !dims_are(*mu, {s.cout}) || !dims_are(*var, {s.cout}))
                return fail(err, IDC_ERR_MISSING_KEY, "BatchNorm '%s' has the wrong shape", s.bnkey);
            float* sc = (float*)(base + lb.bn_scale_off);
            float* sh = (float*)(base + lb.bn_shift_off);
            for (int c = 0; c < cout_pad(s.cout); ++c) { sc[c] = 1.f; sh[c] = 0.f; }
            for (int c = 0; c < s.cout; ++c) {      // eval-BN folded in fp64: y = x*s + t  (eps 1e-5)
                const double sd_ = (double)g->data[c] / sqrt((double)var->data[c] + 1e-5);
                sc[c] = (float)sd_;
                sh[c] = (float)((double)be->data[c] - (double)mu->data[c] * sd_);
                if (a_out[li]) { sc[c] = ldexpf(sc[c], a_out[li]); sh[c] = ldexpf(sh[c], a_out[li]); }      // (after the rounding to fp32: exact)
            }
        }
    }
    run_pack_tasks(tasks);
    // layers that sum a shortcut branch: bias of the fused launch = own bias + the shortcut conv's bias
    for (size_t li = 0; li < plan.active.size(); ++li) {
        const LayerSpec& s = specs[plan.active[li]];
        if (plan.layers[li].fbias_off == (size_t)-1) continue;
        float* fb = (float*)(base + plan.layers[li].fbias_off);
        const float* own = (const float*)(base + plan.layers[li].bias_off);
        for (int ch = 0; ch < cout_pad(s.cout); ++ch) fb[ch] = own[ch];
        for (size_t lj = 0; lj < plan.active.size(); ++lj)
            if (strcmp(specs[plan.active[lj]].name, s.resid) == 0) {
                const float* sb = (const float*)(base + plan.layers[lj].bias_off);
                for (int ch = 0; ch < cout_pad(s.cout); ++ch) fb[ch] += sb[ch];
            }
    }
    {
        const TensorView *w = nullptr, *b = nullptr;
        if (!need("model_out.0.weight", &w) || !dims_are(*w, {2, 128, 1, 1}))
            return fail(err, IDC_ERR_MISSING_KEY, "missing or mis-shaped key 'model_out.0.weight'");
        if (!need("model_out.0.bias", &b) || !dims_are(*b, {2}))
            return fail(err, IDC_ERR_MISSING_KEY, "missing or mis-shaped key 'model_out.0.bias'");
        memcpy(base + plan.head_w_off, w->data, 2 * 128 * 4);
        memcpy(base + plan.head_b_off, b->data, 2 * 4);
    }
    if (plan.pred_ab_off != (size_t)-1) {      // pred_ab: 1x1 conv 313 -> 2 (deploy_nopred.prototxt:842-850; weight = pts_in_hull.T)
        const TensorView *w = nullptr, *b = nullptr;
        if (!need("pred.pred_ab.weight", &w) || !dims_are(*w, {2, 313, 1, 1}))
            return fail(err, IDC_ERR_MISSING_KEY, "missing or mis-shaped key 'pred.pred_ab.weight' (2,313,1,1: the ab bin centres)");
        if (!need("pred.pred_ab.bias", &b) || !dims_are(*b, {2}))
            return fail(err, IDC_ERR_MISSING_KEY, "missing or mis-shaped key 'pred.pred_ab.bias'");
        memcpy(base + plan.pred_ab_off, w->data, 2 * 313 * 4);
        memcpy(base + plan.pred_ab_off + 2 * 313 * 4, b->data, 2 * 4);
    }
    if (plan.glob_off != (size_t)-1) {
        // Global-hints branch (deploy_nodist.prototxt:37-172): stage 1 = glob_conv1 (314 in) + s_conv1 (2 in) summed
        // before the ReLU (Eltwise :66-72), stages 2..4 = glob_conv2..4; each followed by ReLU then BatchNorm.
        // Stored transposed [k][512] + (bias, bn scale, bn shift) per stage, all fp32.
        float* gp = (float*)(base + plan.glob_off);
        auto conv1x1 = [&](const char* key, int cin, const TensorView** w, const TensorView** b) -> bool {
            const std::string wk = std::string(key) + ".weight", bk = std::string(key) + ".bias";
            return need(wk, w) && need(bk, b) && dims_are(**w, {kGlobC, cin, 1, 1}) && dims_are(**b, {kGlobC});
        };
        auto bn_fold = [&](const char* key, float* sc, float* sh) -> bool {
            const TensorView *g = nullptr, *be = nullptr, *mu = nullptr, *var = nullptr;
            const std::string p = key;
            if (!need(p + ".weight", &g) || !need(p + ".bias", &be) || !need(p + ".running_mean", &mu) ||
                !need(p + ".running_var", &var)) return false;
            if (!dims_are(*g, {kGlobC}) || !dims_are(*be, {kGlobC}) || !dims_are(*mu, {kGlobC}) || !dims_are(*var, {kGlobC})) return false;
            for (int c = 0; c < kGlobC; ++c) {
                const double sd_ = (double)g->data[c] / sqrt((double)var->data[c] + 1e-5);
                sc[c] = (float)sd_; sh[c] = (float)((double)be->data[c] - (double)mu->data[c] * sd_);
            }
            return true;
        };
        const TensorView *wg = nullptr, *bg = nullptr, *ws = nullptr, *bs = nullptr;
        if (!conv1x1("glob.glob_conv1", 314, &wg, &bg) || !conv1x1("glob.s_conv1", 2, &ws, &bs))
            return fail(err, IDC_ERR_MISSING_KEY, "missing or mis-shaped global-hints keys 'glob.glob_conv1' / 'glob.s_conv1'");
        for (int k = 0; k < 314; ++k) for (int c = 0; c < kGlobC; ++c) gp[(size_t)k * kGlobC + c] = wg->data[(size_t)c * 314 + k];
        for (int k = 0; k < 2; ++k) for (int c = 0; c < kGlobC; ++c) gp[(size_t)(314 + k) * kGlobC + c] = ws->data[(size_t)c * 2 + k];
        float* q = gp + (size_t)kGlobIn * kGlobC;
        for (int c = 0; c < kGlobC; ++c) q[c] = bg->data[c] + bs->data[c];
        if (!bn_fold("glob.bn1", q + kGlobC, q + 2 * kGlobC))
            return fail(err, IDC_ERR_MISSING_KEY, "missing or mis-shaped BatchNorm keys under 'glob.bn1'");
        q += 3 * kGlobC;
        for (int st = 2; st <= 4; ++st) {
            char ck[32], bk[32];
            snprintf(ck, sizeof(ck), "glob.glob_conv%d", st); snprintf(bk, sizeof(bk), "glob.bn%d", st);
            const TensorView *w = nullptr, *b = nullptr;
            if (!conv1x1(ck, kGlobC, &w, &b)) return fail(err, IDC_ERR_MISSING_KEY, "missing or mis-shaped key '%s'", ck);
            for (int k = 0; k < kGlobC; ++k) for (int c = 0; c < kGlobC; ++c) q[(size_t)k * kGlobC + c] = w->data[(size_t)c * kGlobC + k];
            float* r = q + (size_t)kGlobC * kGlobC;
            for (int c = 0; c < kGlobC; ++c) r[c] = b->data[c];
            if (!bn_fold(bk, r + kGlobC, r + 2 * kGlobC)) return fail(err, IDC_ERR_MISSING_KEY, "missing or mis-shaped BatchNorm keys under '%s'", bk);
            q = r + 3 * kGlobC;
        }
    }
    BlobHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = kBlobMagic; h.version = IDC_VERSION; h.precision = (uint32_t)precision; h.flags = plan.flags;
    for (size_t li = 0; li < a_out.size(); ++li)
        if (a_out[li] != 0) { h.flags |= kBlobFlagActExp; h.pad[li] = (uint8_t)(int8_t)a_out[li]; }
    h.total_bytes = plan.total_bytes;
    h.checksum = fnv1a(base + sizeof(BlobHeader), plan.total_bytes - sizeof(BlobHeader));
    memcpy(base, &h, sizeof(h));
    return IDC_OK;
}

static int validate_header(idc_context* h, const BlobHeader& hd, size_t blob_bytes) {
    if (hd.magic != kBlobMagic || hd.version != IDC_VERSION)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "not an ideepcolor weight blob (bad magic/version)");
    const bool with_exp = (hd.flags & kBlobFlagActExp) != 0;        // packed with activation exponents: not a handle flag, IDC_FP16X3 blobs only
    if ((int)hd.precision != h->precision || (hd.flags & ~kBlobFlagActExp) != h->plan.flags)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "blob was packed for precision %u flags %u%s, handle needs %d/%u",
                    hd.precision, hd.flags & ~kBlobFlagActExp, with_exp ? " (+ activation exponents)" : "", h->precision, h->plan.flags);
    if (with_exp && (h->precision != IDC_FP16X3 || h->plan.active.size() > sizeof(hd.pad)))
        return fail(&h->err, IDC_ERR_INVALID_ARG, "blob carries activation exponents (header flag 0x%x): only IDC_FP16X3 handles without head flags take them", kBlobFlagActExp);
    if (hd.total_bytes != h->plan.total_bytes || blob_bytes < h->plan.total_bytes)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "blob size mismatch");
    return IDC_OK;
}

// What the host side needs to know about the blob in use: the activation exponent of every active layer (header) and the accumulator-scale words
// (the fused deconv + shortcut launch checks that its two layers agree before it shares one).  host_blob: the whole validated blob in host memory.
static void cache_blob_meta(idc_context* h, const uint8_t* host_blob) {
    BlobHeader hd;
    memcpy(&hd, host_blob, sizeof(hd));
    const size_t nl = h->plan.active.size();
    h->act_exp.assign(nl, 0); h->wscale.assign(nl, 1.f);
    for (size_t li = 0; li < nl; ++li) {
        if ((hd.flags & kBlobFlagActExp) && li < sizeof(hd.pad)) h->act_exp[li] = (int)(int8_t)hd.pad[li];
        if (h->plan.layers[li].wscale_off != (size_t)-1) memcpy(&h->wscale[li], host_blob + h->plan.layers[li].wscale_off, 4);
    }
}

// header + payload checksum of a packed blob in device memory: one D2H copy at load time (136 MB, a few ms) -- a
// truncated or stale broadcast must not become silent garbage weights
int verify_device_blob(idc_context* h, const void* dev_blob, size_t blob_bytes) {
    BlobHeader hd;
    if (blob_bytes < sizeof(hd)) return fail(&h->err, IDC_ERR_INVALID_ARG, "blob too small");
    HIPCHK(h, hipMemcpy(&hd, dev_blob, sizeof(hd), hipMemcpyDeviceToHost));
    int rc = validate_header(h, hd, blob_bytes);
    if (rc) return rc;
    std::vector<uint8_t> tmp(h->plan.total_bytes);
    HIPCHK(h, hipMemcpy(tmp.data(), dev_blob, tmp.size(), hipMemcpyDeviceToHost));
    if (fnv1a(tmp.data() + sizeof(hd), tmp.size() - sizeof(hd)) != hd.checksum)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "device blob checksum mismatch");
    cache_blob_meta(h, tmp.data());
    return IDC_OK;
}

int own_blob_storage(idc_context* h) {
    const hipError_t e = h->blob_mem.ensure(h->plan.total_bytes);
    h->d_blob = h->blob_mem.get();
    HIPCHK(h, e);
    return IDC_OK;
}

}  // namespace idc

extern "C" {

size_t idc_weights_blob_bytes(int precision, unsigned flags) {
    if (precision < IDC_FP32 || precision > IDC_FP16) return 0;
    return make_blob_plan(precision, flags).total_bytes;
}

int idc_pack_weights(int precision, unsigned flags, const idc_tensor_desc* tensors, int n_tensors, void* blob,
                     size_t blob_bytes) {
    return pack_weights_impl(precision, flags, tensors, n_tensors, blob, blob_bytes, nullptr);
}

int idc_set_weights_host(idc_handle h, const void* blob, size_t blob_bytes) {
    if (!h || !blob) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null handle/blob");
    BlobHeader hd;
    if (blob_bytes < sizeof(hd)) return fail(&h->err, IDC_ERR_INVALID_ARG, "blob too small");
    memcpy(&hd, blob, sizeof(hd));
    int rc = validate_header(h, hd, blob_bytes);
    if (rc) return rc;
    if (fnv1a((const uint8_t*)blob + sizeof(hd), h->plan.total_bytes - sizeof(hd)) != hd.checksum)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "blob checksum mismatch");
    HIPCHK(h, hipSetDevice(h->device));
    rc = own_blob_storage(h);
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(h->blob_mem.get(), blob, h->plan.total_bytes, hipMemcpyHostToDevice));
    cache_blob_meta(h, (const uint8_t*)blob);
    h->weights_set = true;
    return IDC_OK;
}

int idc_set_weights_device(idc_handle h, const void* dev_blob, size_t blob_bytes, int copy) {
    if (!h || !dev_blob) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null handle/blob");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = verify_device_blob(h, dev_blob, blob_bytes);
    if (rc) return rc;
    if (copy) {
        rc = own_blob_storage(h);
        if (rc) return rc;
        HIPCHK(h, hipMemcpy(h->blob_mem.get(), dev_blob, h->plan.total_bytes, hipMemcpyDeviceToDevice));
    } else {
        h->blob_mem.reset();
        h->d_blob = (const uint8_t*)dev_blob;
    }
    h->weights_set = true;
    return IDC_OK;
}

int idc_pack_weights_ex(int precision, unsigned flags, const idc_tensor_desc* tensors, int n_tensors, const int* act_exp, int n_layers,
                        void* blob, size_t blob_bytes) {
    return pack_weights_impl(precision, flags, tensors, n_tensors, blob, blob_bytes, nullptr, act_exp, n_layers);
}

int idc_load_weights_ex(idc_handle h, const idc_tensor_desc* tensors, int n_tensors, const int* act_exp, int n_layers) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    std::vector<uint8_t> blob(h->plan.total_bytes);
    int rc = pack_weights_impl(h->precision, h->flags, tensors, n_tensors, blob.data(), blob.size(), &h->err, act_exp, n_layers);
    if (rc) return rc;
    return idc_set_weights_host(h, blob.data(), blob.size());
}

int idc_load_weights(idc_handle h, const idc_tensor_desc* tensors, int n_tensors) {
    return idc_load_weights_ex(h, tensors, n_tensors, nullptr, 0);
}

const void* idc_weights_device_ptr(idc_handle h) { return (h && h->weights_set) ? h->d_blob : nullptr; }

}  // extern "C"
