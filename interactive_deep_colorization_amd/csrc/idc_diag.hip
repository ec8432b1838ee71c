// idc_diag.hip -- looking inside a handle (C ABI, include/ideepcolor.h): the layer table (idc_layer_info_get), the range audit, per-layer profiling,
// idc_get_activation, and the single-operator entry points the tests use to run one conv / deconv exactly as the network would plan it.
// Nothing here is on a forward's path.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "idc_engine.h"

extern "C" {

int idc_num_layers(idc_handle h) { return h ? h->n_timed : 0; }

int idc_layer_info_get(idc_handle h, int layer, idc_layer_info* out) {
    if (!h || !out) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null argument");
    if (layer < 0 || layer >= h->n_timed) return fail(&h->err, IDC_ERR_INVALID_ARG, "layer %d out of range", layer);
    memset(out, 0, sizeof(*out));
    const int nl = (int)h->layers.size();
    const double hw = (double)h->H * h->W;
    const int eb = elem_bytes(h->precision);
    if (layer == 0) {
        snprintf(out->name, sizeof(out->name), "glob_branch");
        snprintf(out->kernel, sizeof(out->kernel), (h->flags & IDC_FLAG_GLOBAL_HINTS) ? "glob_branch_kernel" : "(input pack fused into conv1_1)");
        out->min_bytes = 0; out->launches = (h->flags & IDC_FLAG_GLOBAL_HINTS) ? 1 : 0;
    } else if (layer <= nl) {
        const Layer& L = h->layers[layer - 1];
        snprintf(out->name, sizeof(out->name), "%s", L.spec->name);
        if (L.kernel == kFused) {            // its MACs and bytes are accounted to the launch that runs them
            for (const Layer& C : h->layers)
                if (C.fused_short == layer - 1 || C.fused_next == layer - 1) snprintf(out->kernel, sizeof(out->kernel), "fused into %s", C.spec->name);
            out->flops = 0; out->min_bytes = 0; out->launches = 0;
        } else if (L.chained_into >= 0) {    // ran inside the persistent trunk launch headed by another layer (its own MACs stay its own)
            snprintf(out->kernel, sizeof(out->kernel), "chained into %s", h->layers[L.chained_into].spec->name);
            out->flops = L.flops; out->min_bytes = L.min_bytes; out->launches = 0;
        } else if (L.chain_len > 0) {
            snprintf(out->kernel, sizeof(out->kernel), "conv_kwave_chain_bf16 x%d", L.chain_len);
            out->flops = L.flops; out->min_bytes = L.min_bytes; out->launches = 1;
        } else {
            kernel_label(L, h->precision, out->kernel, sizeof(out->kernel));
            out->flops = L.flops; out->min_bytes = L.min_bytes; out->launches = 1;
            if (L.fused_next >= 0) {
                const Layer& P = h->layers[L.fused_next];
                out->flops += P.flops;
                out->min_bytes += P.min_bytes - 2.0 * (double)h->tensors[L.dst].H * h->tensors[L.dst].W * h->tensors[L.dst].Cpad * eb;
            }
            if (L.fused_short >= 0) {
                const Layer& P = h->layers[L.fused_short];
                out->flops += P.flops;
                // (the shortcut sums are neither written nor read: fp32 in the operand-split graph, bf16 otherwise)
                out->min_bytes += P.min_bytes - 2.0 * (double)h->tensors[P.dst].H * h->tensors[P.dst].W * h->tensors[P.dst].Cpad * (h->tensors[P.dst].is_f32 ? 4 : eb);
            }
        }
    } else if (layer == nl + 1) {
        snprintf(out->name, sizeof(out->name), "head");
        snprintf(out->kernel, sizeof(out->kernel), "head_kernel");
        out->flops = 2.0 * 128 * 2 * hw; out->min_bytes = hw * 128 * eb + hw * 2 * 4; out->launches = 1;
    } else {
        snprintf(out->name, sizeof(out->name), "dist_softmax");
        snprintf(out->kernel, sizeof(out->kernel), "softmax_nchw_kernel");
        out->launches = (h->flags & IDC_FLAG_DIST_HEAD) ? 1 : 0;
        out->min_bytes = out->launches ? (hw / 16) * (640 + 529) * 4 : 0;
    }
    return IDC_OK;
}

int idc_set_range_audit(idc_handle h, int on) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (on && !h->d_audit) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMalloc((void**)&h->d_audit, (size_t)h->n_timed * sizeof(AuditRecord)));
        HIPCHK(h, hipMemsetAsync(h->d_audit, 0, (size_t)h->n_timed * sizeof(AuditRecord), h->stream));
        h->audit_values.assign((size_t)h->n_timed, 0);
    }
    h->audit = on != 0;
    return IDC_OK;
}

int idc_range_reset(idc_handle h) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (h->d_audit) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemsetAsync(h->d_audit, 0, (size_t)h->n_timed * sizeof(AuditRecord), h->stream));     // stream-ordered behind the audited forwards
        h->audit_values.assign((size_t)h->n_timed, 0);
    }
    return IDC_OK;
}

int idc_range_report(idc_handle h, int layer, idc_range_info* out) {
    if (!h || !out) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null argument");
    if (layer < 0 || layer >= h->n_timed) return fail(&h->err, IDC_ERR_INVALID_ARG, "layer %d out of range", layer);
    memset(out, 0, sizeof(*out));
    idc_layer_info info;
    int rc = idc_layer_info_get(h, layer, &info);
    if (rc) return rc;
    snprintf(out->name, sizeof(out->name), "%s", info.name);
    const int nl = (int)h->layers.size();
    if (layer >= 1 && layer <= nl) {
        const Tensor& t = h->tensors[h->layers[layer - 1].dst];
        const bool f32 = t.is_f32 || h->precision == IDC_FP32;
        out->storage = f32 ? IDC_STORE_F32 : (split_is_f16(h->precision) ? IDC_STORE_F16 : IDC_STORE_BF16);
        out->parts = f32 ? 1 : t.parts;
        if ((size_t)(layer - 1) < h->act_exp.size()) out->act_exp = h->act_exp[layer - 1];
    }
    if (!h->d_audit) return IDC_OK;                  // never switched on: all counts zero
    HIPCHK(h, hipSetDevice(h->device));
    AuditRecord r;
    HIPCHK(h, hipMemcpyAsync(&r, h->d_audit + layer, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    rc = check_chain_abort(h);
    if (rc) return rc;
    memcpy(&out->max_abs, &r.max_abs_bits, 4);
    out->n_values = h->audit_values[(size_t)layer];
    out->n_saturated = r.n_saturated; out->n_tiny = r.n_tiny; out->n_nonfinite = r.n_nonfinite;
    if (out->n_values == 0) out->storage = IDC_STORE_NONE;
    return IDC_OK;
}

int idc_set_profiling(idc_handle h, int on) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (on != 0 && h->ev.empty()) {
        HIPCHK(h, hipSetDevice(h->device));
        h->ev.assign((size_t)h->n_timed * 2 * kProfRing, nullptr);
        for (auto& e : h->ev) HIPCHK(h, hipEventCreate(&e));
    }
    h->profiling = on == 2 ? 2 : (on != 0 ? 1 : 0);
    h->prof_count = 0;
    return IDC_OK;
}

int idc_layer_times_ms(idc_handle h, float* ms, int capacity) {
    if (!h || !ms) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null argument");
    if (h->ev.empty()) return fail(&h->err, IDC_ERR_INVALID_ARG, "no forward was recorded with profiling on");
    if (capacity < h->n_timed) return fail(&h->err, IDC_ERR_INVALID_ARG, "capacity %d < %d", capacity, h->n_timed);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int slots = (int)(h->prof_count < kProfRing ? h->prof_count : kProfRing);
    if (slots == 0) return fail(&h->err, IDC_ERR_INVALID_ARG, "no forward was recorded with profiling on");
    for (int i = 0; i < h->n_timed; ++i) {
        if (h->profiling == 2 && i > 0) { ms[i] = 0.f; continue; }       // mode 2: ms[0] = the whole forward
        double sum = 0;
        for (int sl = 0; sl < slots; ++sl) {
            float t = 0.f;
            const size_t base = (size_t)sl * h->n_timed * 2;
            if (hipEventElapsedTime(&t, h->ev[base + i * 2], h->ev[base + i * 2 + 1]) != hipSuccess) { t = 0.f; (void)hipGetLastError(); }
            sum += t;
        }
        ms[i] = (float)(sum / slots);
    }
    return IDC_OK;
}

int idc_layer_times_stats(idc_handle h, float* ms_min, float* ms_median, float* ms_max, int capacity) {
    if (!h || !ms_min || !ms_median || !ms_max) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null argument");
    if (h->ev.empty()) return fail(&h->err, IDC_ERR_INVALID_ARG, "no forward was recorded with profiling on");
    if (capacity < h->n_timed) return fail(&h->err, IDC_ERR_INVALID_ARG, "capacity %d < %d", capacity, h->n_timed);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const int slots = (int)(h->prof_count < kProfRing ? h->prof_count : kProfRing);
    if (slots == 0) return fail(&h->err, IDC_ERR_INVALID_ARG, "no forward was recorded with profiling on");
    std::vector<float> v((size_t)slots);
    for (int i = 0; i < h->n_timed; ++i) {
        if (h->profiling == 2 && i > 0) { ms_min[i] = ms_median[i] = ms_max[i] = 0.f; continue; }
        for (int sl = 0; sl < slots; ++sl) {
            float t = 0.f;
            const size_t base = (size_t)sl * h->n_timed * 2;
            if (hipEventElapsedTime(&t, h->ev[base + i * 2], h->ev[base + i * 2 + 1]) != hipSuccess) { t = 0.f; (void)hipGetLastError(); }
            v[(size_t)sl] = t;
        }
        std::sort(v.begin(), v.end());
        ms_min[i] = v.front(); ms_max[i] = v.back();
        ms_median[i] = (slots & 1) ? v[(size_t)slots / 2] : 0.5f * (v[(size_t)slots / 2 - 1] + v[(size_t)slots / 2]);
    }
    return IDC_OK;
}

int idc_get_activation(idc_handle h, const char* name, int n, float* out, size_t capacity_floats, int* C, int* H,
                       int* W) {
    if (!h || !name || !out) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null argument");
    const int ti = find_tensor(h, name);
    if (ti < 0) return fail(&h->err, IDC_ERR_INVALID_ARG, "no activation named '%s'", name);
    const Tensor& t = h->tensors[ti];
    if (n <= 0 || n > h->max_batch) return fail(&h->err, IDC_ERR_BATCH, "bad n");
    for (size_t li = 0; li < h->layers.size(); ++li) {      // a tensor the last forward never wrote: say so, do not return stale data
        const Layer& L = h->layers[li];
        if (L.dst != ti) continue;
        bool fused_away = L.fused_next >= 0 || L.fused_head; // conv1_1 inside conv1_block_fused; conv10_2 consumed by the head in its own epilogue
        for (const Layer& C : h->layers) fused_away = fused_away || C.fused_short == (int)li;   // shortcut conv inside conv_ds_fused
        if (fused_away)
            return fail(&h->err, IDC_ERR_UNSUPPORTED, "activation '%s' is not materialised: its layer runs fused inside another "
                        "launch (idc_set_option(\"fuse_conv1\", 0) / IDC_FUSE_SHORTCUT=0 keep the launches apart)", name);
    }
    const size_t need = (size_t)n * t.C * t.H * t.W;
    if (capacity_floats < need) return fail(&h->err, IDC_ERR_INVALID_ARG, "need %zu floats", need);
    HIPCHK(h, hipSetDevice(h->device));
    if (h->scratch_bytes < need * 4) {
        if (h->d_scratch) (void)hipFree(h->d_scratch);
        h->d_scratch = nullptr; h->scratch_bytes = 0;
        HIPCHK(h, hipMalloc((void**)&h->d_scratch, need * 4));
        h->scratch_bytes = need * 4;
    }
    const int src_bf16 = (!t.is_f32 && h->precision != IDC_FP32) ? 1 : 0;
    if (t.parts > 1 || (is_split(h->precision) && !t.is_f32)) HIPCHK(h, launch_split_to_nchw(      // (IDC_FP16: one fp16 plane)
        t.ptr, h->d_scratch, n, t.C, t.H, t.W, t.Cpad, t.parts, split_is_f16(h->precision) ? 1 : 0, h->stream));
    else HIPCHK(h, launch_nhwc_to_nchw(src_bf16, t.ptr, h->d_scratch, n, t.C, t.H, t.W, t.Cpad, h->stream));
    HIPCHK(h, hipMemcpyAsync(out, h->d_scratch, need * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t li = 0; li < h->layers.size() && li < h->act_exp.size(); ++li)      // stored as value * 2^a: hand out the value (a power of two: exact)
        if (h->layers[li].dst == ti && h->act_exp[li] != 0)
            for (size_t i = 0; i < need; ++i) out[i] = ldexpf(out[i], -h->act_exp[li]);
    if (C) *C = t.C;
    if (H) *H = t.H;
    if (W) *W = t.W;
    return IDC_OK;
}

// ---- single operators -----------------------------------------------------------------------------

// the kernel_label of the launch the last single-operator call on this thread made (idc_op_last_kernel); a conv_ds_fused_m / _mh launch also says
// which of its two forms ran (" half" = 64 couts, 4 waves; " 8-wave"), which the layer table's label leaves to the grid
static thread_local std::string g_op_last_kernel;

// the 3x3 shortcut conv that rides in a deconv's launch (idc_op_deconv_shortcut): x [n, cin, 2h, 2w], w [cout, cin, 3, 3], b [cout]
struct ShortcutOp { int cin; const float* x; const float* w; const float* b; };

static int run_single_op(int device_id, int precision, LayerSpec spec, int n, int h, int w, const float* x,
                         const float* weight, const float* bias, const float* bn_scale, const float* bn_shift,
                         const float* resid, float* y, const ShortcutOp* sc = nullptr) {
    g_op_last_kernel.clear();
    int rc = check_device(device_id, nullptr);
    if (rc) return rc;
    if (precision < IDC_FP32 || precision > IDC_FP16) return fail(nullptr, IDC_ERR_INVALID_ARG, "bad precision");
    if (!x || !weight || !bias || !y || n <= 0 || h <= 0 || w <= 0) return fail(nullptr, IDC_ERR_INVALID_ARG, "bad argument");
    const bool split = is_split(precision);
    const int parts = split_parts(precision);
    if (split && !v2_eligible(spec)) return fail(nullptr, IDC_ERR_UNSUPPORTED, "operand-split precisions run the large tile only: cout >= 65");
    const int kc = kc_elems(precision), eb = elem_bytes(precision);
    if (spec.cin % kc) return fail(nullptr, IDC_ERR_UNSUPPORTED, "cin must be a multiple of %d in this precision", kc);
    if (spec.in_stride != 1 && spec.in_stride != 2) return fail(nullptr, IDC_ERR_INVALID_ARG, "in_stride must be 1 or 2");
    if (h % spec.in_stride || w % spec.in_stride) return fail(nullptr, IDC_ERR_INVALID_ARG, "H, W must divide by in_stride");
    if (sc && (!sc->x || !sc->w || !sc->b || sc->cin <= 0 || sc->cin % kc)) return fail(nullptr, IDC_ERR_INVALID_ARG, "bad shortcut operand");
    // the batch the variant is chosen for, as a handle's max_batch is (option "op_policy_batch"; 0 = this call's own batch); the launch carries n
    const int n_policy = options().op_policy_batch > 0 ? options().op_policy_batch : n;
    idc_context* nullctx = nullptr;
    HIPCHK(nullctx, hipSetDevice(device_id));
    HIPCHK(nullctx, init_kernels());
    Layer L;
    // the shortcut sum arrives through the `resid` pointer; every eligibility gate of set_geometry reads spec.resid (a 3x3 op with
    // a residual must not be handed to conv_kwave_bf16 / the Winograd forms, which do not take one -- ADVICE r4)
    spec.resid = resid ? "resid" : nullptr;
    // ... and spec.out_f32: the op stores fp32 on the fp32 path only (a.out_f32 below); left at 1, the default library's planner kept every
    // bf16 op off the large tile, which writes bf16 only, whatever the tile policy asked for
    spec.out_f32 = (precision == IDC_BF16 || split) ? 0 : 1;
    L.spec = &spec;
    L.blob.nkc = spec.cin / kc; L.blob.ncg = cout_pad(spec.cout) / kCoutGroup;
    L.blob.w_bytes = (size_t)weight_taps(spec.kind) * L.blob.nkc * L.blob.ncg * kWBlockBytes;
    L.blob.w_off = 0; L.blob.w2_off = (size_t)-1; L.blob.bias_off = L.blob.bn_scale_off = L.blob.bn_shift_off = L.blob.fbias_off = (size_t)-1;
    const int cpad = cout_pad(spec.cout);
    // fp32 3x3 stride-1 ops without a shortcut sum take the Winograd kernel exactly as inside the network
    const bool wino_dc = !split && wino_deconv_eligible(spec) && spec.cin % kc == 0;
    const bool wino_ok = !split && ((wino_eligible(spec) && spec.cin % kc == 0 && resid == nullptr) || wino_dc);
    L.blob.w3_off = wino_ok ? 0 : (size_t)-1;
    L.blob.w3_bytes = wino_ok ? (size_t)spec.cin * cpad * (wino_dc ? 36 : 16) * eb : 0;
    const size_t wimg_bytes = std::max(L.blob.w_bytes * parts, L.blob.w3_bytes);             // one staging buffer serves either image
    L.lprec = precision; L.split = split;
    const int Hs = h / spec.in_stride, Ws = w / spec.in_stride;
    const int so = spec.kind == kDeconv4x4 ? 2 : 1;
    const int Ho = Hs * so, Wo = Ws * so;
    fill_taps(L);
    // (default library: the large tile only where conv_igemm_v2m / v2p cover the launch -- no shortcut sum, no LeakyReLU without the fused head)
    set_geometry(L, precision, n, n_policy, Hs, Ws, kAbPartners || is_split(precision) || (resid == nullptr && spec.act != 2));
    const size_t wcount = (size_t)spec.cin * spec.cout * (spec.kind == kDeconv4x4 ? 16 : spec.kind == kConv1x1 ? 1 : 9);
    int op_wexp = (split_is_f16(precision) && parts > 1) ? f16_weight_exponent(weight, wcount) : 0;      // as the blob packer does per layer
    // deconv + shortcut conv in one launch: run_graph's conditions for the pair (the large tile, conv_ds_fused's domain), else the network runs two launches
    LayerSpec spec2{"op_short", "op_short", nullptr, kConv3x3, sc ? sc->cin : 0, spec.cout, 1, 1, 0, "x_short", nullptr, 1, 1, 0};
    LayerBlob blob2 = L.blob;
    if (sc) {
        blob2.nkc = sc->cin / kc;
        blob2.w_bytes = (size_t)weight_taps(kConv3x3) * blob2.nkc * blob2.ncg * kWBlockBytes;
        const bool fits = split ? conv_ds_m_fits(Hs, Ws, L.blob.nkc * parts, blob2.nkc * parts) : conv_ds_m_fits(Hs, Ws, L.blob.nkc, blob2.nkc);
        if (L.kernel != kConvV2 || !fuse_shortcut_enabled() || (split && !options().split_ds_fuse) || spec.cout % 128 != 0 || spec.act == 2 ||
            (!kAbPartners && !split && !(options().ds_m16 != 0 && fits)) || (split && !fits))
            return fail(nullptr, IDC_ERR_UNSUPPORTED, "deconv + shortcut: the network runs this pair as two launches here (policy batch %d, options)", n_policy);
        L.fused_short = 0;
        if (split_is_f16(precision) && parts > 1) {      // one accumulator set, one accumulator scale: the smaller of the two weight exponents, as the blob packer does
            const int e2 = f16_weight_exponent(sc->w, (size_t)sc->cin * spec.cout * 9);
            if (e2 < op_wexp) op_wexp = e2;
        }
    }
    std::vector<float> hb(cpad, 0.f), hs(cpad, 1.f), ht(cpad, 0.f);
    for (int c = 0; c < spec.cout; ++c) {
        hb[c] = bias[c] + (sc ? sc->b[c] : 0.f);
        if (bn_scale) { hs[c] = bn_scale[c]; ht[c] = bn_shift ? bn_shift[c] : 0.f; }
    }
    DevBuf d_x, d_xn, d_w, d_b, d_s, d_t, d_r, d_rn, d_yn, d_y, d_x2, d_x2n, d_w2;
    const size_t xin = (size_t)n * spec.cin * h * w, yout = (size_t)n * spec.cout * Ho * Wo;
    HIPCHK(nullctx, d_x.alloc(xin * 4));
    HIPCHK(nullctx, d_xn.alloc(xin * eb * parts));
    HIPCHK(nullctx, d_w.alloc(wimg_bytes));
    HIPCHK(nullctx, d_b.alloc(cpad * 4)); HIPCHK(nullctx, d_s.alloc(cpad * 4)); HIPCHK(nullctx, d_t.alloc(cpad * 4));
    HIPCHK(nullctx, d_yn.alloc((size_t)n * Ho * Wo * cpad * (split ? 2 * parts : 4)));
    HIPCHK(nullctx, d_y.alloc(yout * 4));
    HIPCHK(nullctx, hipMemcpy(d_x.p, x, xin * 4, hipMemcpyHostToDevice));
    HIPCHK(nullctx, hipMemcpy(d_b.p, hb.data(), cpad * 4, hipMemcpyHostToDevice));
    HIPCHK(nullctx, hipMemcpy(d_s.p, hs.data(), cpad * 4, hipMemcpyHostToDevice));
    HIPCHK(nullctx, hipMemcpy(d_t.p, ht.data(), cpad * 4, hipMemcpyHostToDevice));
    if (split) HIPCHK(nullctx, launch_nchw_to_split((const float*)d_x.p, d_xn.p, n, spec.cin, h, w, spec.cin, parts, split_is_f16(precision) ? 1 : 0, nullptr));
    else HIPCHK(nullctx, launch_nchw_to_nhwc(precision, (const float*)d_x.p, d_xn.p, n, spec.cin, h, w, spec.cin, nullptr));
    // bf16 precision: the residual arrives and the output leaves in bf16, as inside the network (operand-split: fp32 residual, split output)
    const int io_bf16 = precision == IDC_BF16 ? 1 : 0;
    if (resid) {
        HIPCHK(nullctx, d_r.alloc(yout * 4));
        HIPCHK(nullctx, d_rn.alloc((size_t)n * Ho * Wo * cpad * 4));
        HIPCHK(nullctx, hipMemcpy(d_r.p, resid, yout * 4, hipMemcpyHostToDevice));
        HIPCHK(nullctx, launch_nchw_to_nhwc(io_bf16, (const float*)d_r.p, d_rn.p, n, spec.cout, Ho, Wo, cpad, nullptr));
    }
    ConvArgs& a = L.args;
    a.in = d_xn.p; a.out = d_yn.p; a.wgt = d_w.p; a.bias = (const float*)d_b.p;
    a.bn_scale = bn_scale ? (const float*)d_s.p : nullptr;
    a.bn_shift = bn_scale ? (const float*)d_t.p : nullptr;
    a.resid = resid ? d_rn.p : nullptr;
    a.resid_bf16 = io_bf16;
    a.head_w = nullptr; a.head_b = nullptr; a.head_out = nullptr; a.head_mul = 0.f;
    a.in2 = nullptr; a.wgt2 = nullptr; a.nkc2 = 0;
    if (sc) {              // bound as run_graph binds a layer's fused_short
        const size_t x2n = (size_t)n * sc->cin * Ho * Wo;
        HIPCHK(nullctx, d_x2.alloc(x2n * 4));
        HIPCHK(nullctx, d_x2n.alloc(x2n * eb * parts));
        HIPCHK(nullctx, d_w2.alloc(blob2.w_bytes * parts));
        HIPCHK(nullctx, hipMemcpy(d_x2.p, sc->x, x2n * 4, hipMemcpyHostToDevice));
        if (split) HIPCHK(nullctx, launch_nchw_to_split((const float*)d_x2.p, d_x2n.p, n, sc->cin, Ho, Wo, sc->cin, parts, split_is_f16(precision) ? 1 : 0, nullptr));
        else HIPCHK(nullctx, launch_nchw_to_nhwc(precision, (const float*)d_x2.p, d_x2n.p, n, sc->cin, Ho, Wo, sc->cin, nullptr));
        a.in2 = d_x2n.p; a.wgt2 = d_w2.p; a.nkc2 = blob2.nkc;
        if (split) a.w_part_bytes2 = blob2.w_bytes;
    }
    a.warm = options().code_warm;
    a.split_f16 = split_is_f16(precision) ? 1 : 0;
    a.out_f32 = (io_bf16 || split) ? 0 : 1;
    if (split) {
        a.in_parts = parts; a.out_parts = parts; a.nseg = split_segments(precision); a.seg_x = split_seg_x(precision); a.seg_w = split_seg_w(precision);
        a.w_part_bytes = L.blob.w_bytes;
    }
    DevBuf d_part, d_zero, d_wsc;
    a.acc_scale = nullptr;
    if (split && split_is_f16(precision)) {
        const float sc = ldexpf(1.f, -op_wexp);
        HIPCHK(nullctx, d_wsc.alloc(256));
        HIPCHK(nullctx, hipMemcpy(d_wsc.p, &sc, 4, hipMemcpyHostToDevice));
        a.acc_scale = (const float*)d_wsc.p;
    }
    if (a.ksplit > 1) {
        HIPCHK(nullctx, d_part.alloc((size_t)a.ksplit * n * Ho * Wo * cpad * 4));
        a.partial = (float*)d_part.p;
    }
    HIPCHK(nullctx, d_zero.alloc(256));
    HIPCHK(nullctx, hipMemset(d_zero.p, 0, 256));
    a.zeros = d_zero.p;
    // the kernel the network launches for this layer at batch n, and the weight image it reads
    L.kernel = choose_kernel(L, precision, n_policy);
    if (sc) {
        if (L.kernel == kConvDs) return fail(nullptr, IDC_ERR_UNSUPPORTED, "deconv + shortcut: conv_ds_fused (the 32x32x16-MFMA partner) has no single-operator entry");
        std::vector<uint8_t> wimg2(blob2.w_bytes * parts);
        for (int part = 0; part < parts; ++part)
            pack_layer_weights(wimg2.data() + (size_t)part * blob2.w_bytes, precision, 1, spec2, blob2, sc->w, part, ldexpf(1.f, op_wexp));
        HIPCHK(nullctx, hipMemcpy(d_w2.p, wimg2.data(), wimg2.size(), hipMemcpyHostToDevice));
    }
    {
        char k[64]; kernel_label(L, precision, k, sizeof(k));
        g_op_last_kernel = k;
        if (L.kernel == kConvDsM) g_op_last_kernel += conv_ds_m_half(a) ? " half" : " 8-wave";
    }
    std::vector<uint8_t> wimg(wimg_bytes);
    if (L.kernel == kDeconvWino) pack_wino_deconv_weights(wimg.data(), precision, spec, L.blob, weight);
    else if (L.kernel == kConvWino) pack_wino_weights(wimg.data(), precision, spec, L.blob, weight);
    else
        for (int part = 0; part < parts; ++part)
            pack_layer_weights(wimg.data() + (size_t)part * L.blob.w_bytes, precision, L.kernel == kConvV2 ? 2 : 1, spec, L.blob, weight, part, ldexpf(1.f, op_wexp));
    HIPCHK(nullctx, hipMemcpy(d_w.p, wimg.data(), wimg_bytes, hipMemcpyHostToDevice));
    const hipError_t le = launch_kernel(L.kernel, L, a, nullptr);
    if (le == hipErrorInvalidConfiguration) {
        char k[64]; kernel_label(L, precision, k, sizeof(k));
        return fail(nullptr, IDC_ERR_INTERNAL, "single op: %s planned for a launch it does not cover", k);
    }
    HIPCHK(nullctx, le);
    if (a.ksplit > 1) HIPCHK(nullctx, launch_splitk_epilogue(precision, a, nullptr));
    if (split) HIPCHK(nullctx, launch_split_to_nchw(d_yn.p, (float*)d_y.p, n, spec.cout, Ho, Wo, cpad, parts, split_is_f16(precision) ? 1 : 0, nullptr));
    else HIPCHK(nullctx, launch_nhwc_to_nchw(io_bf16, d_yn.p, (float*)d_y.p, n, spec.cout, Ho, Wo, cpad, nullptr));
    HIPCHK(nullctx, hipMemcpy(y, d_y.p, yout * 4, hipMemcpyDeviceToHost));
    HIPCHK(nullctx, hipDeviceSynchronize());
    return IDC_OK;
}

int idc_op_conv2d(int device_id, int precision, int n, int cin, int h, int w, const float* x, int cout, int ksize,
                  int dilation, int in_stride, const float* weight, const float* bias, int act, const float* bn_scale,
                  const float* bn_shift, const float* resid, float* y) {
    if (ksize != 3 && ksize != 1) return fail(nullptr, IDC_ERR_UNSUPPORTED, "ksize must be 1 or 3");
    if (dilation != 1 && dilation != 2) return fail(nullptr, IDC_ERR_UNSUPPORTED, "dilation must be 1 or 2");
    if (ksize == 1 && (dilation != 1 || in_stride != 1)) return fail(nullptr, IDC_ERR_UNSUPPORTED, "1x1 conv: d=1, stride 1 only");
    LayerSpec s{"op", "op", nullptr, ksize == 3 ? kConv3x3 : kConv1x1, cin, cout, dilation, in_stride, act,
                "x", nullptr, 1, 1, 0};
    return run_single_op(device_id, precision, s, n, h, w, x, weight, bias, bn_scale, bn_shift, resid, y);
}

int idc_op_last_kernel(char* out, int cap) {
    if (!out || cap <= 0) return fail(nullptr, IDC_ERR_INVALID_ARG, "null / empty label buffer");
    snprintf(out, (size_t)cap, "%s", g_op_last_kernel.c_str());
    return IDC_OK;
}

int idc_op_deconv_shortcut(int device_id, int precision, int n, int cin, int h, int w, const float* x, int cout, const float* w_deconv,
                           const float* b_deconv, int cin_short, const float* x_short, const float* w_short, const float* b_short, int act, float* y) {
    LayerSpec s{"op", "op", nullptr, kDeconv4x4, cin, cout, 1, 1, act, "x", nullptr, 1, 1, 0};
    const ShortcutOp sc{cin_short, x_short, w_short, b_short};
    return run_single_op(device_id, precision, s, n, h, w, x, w_deconv, b_deconv, nullptr, nullptr, nullptr, y, &sc);
}

int idc_op_deconv4x4s2(int device_id, int precision, int n, int cin, int h, int w, const float* x, int cout,
                       const float* weight, const float* bias, int act, const float* resid, float* y) {
    LayerSpec s{"op", "op", nullptr, kDeconv4x4, cin, cout, 1, 1, act, "x", nullptr, 1, 1, 0};
    return run_single_op(device_id, precision, s, n, h, w, x, weight, bias, nullptr, nullptr, resid, y);
}

}  // extern "C"
