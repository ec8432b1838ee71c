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

namespace idc {

// Row `layer` of the layer table (0 = the global-hints branch, then the layers, the head, the 529-bin softmax) as the last plan_forward left it
void layer_row(const std::vector<Layer>& layers, const std::vector<Tensor>& tensors, int precision, unsigned flags, int H, int W, int layer, idc_layer_info* out) {
    memset(out, 0, sizeof(*out));
    const int nl = (int)layers.size();
    const double hw = (double)H * W;
    const int eb = elem_bytes(precision);
    if (layer == 0) {
        snprintf(out->name, sizeof(out->name), "glob_branch");
        snprintf(out->kernel, sizeof(out->kernel), (flags & IDC_FLAG_GLOBAL_HINTS) ? "glob_branch_kernel" : "(input pack fused into conv1_1)");
        out->min_bytes = 0; out->launches = (flags & IDC_FLAG_GLOBAL_HINTS) ? 1 : 0;
    } else if (layer <= nl) {
        const Layer& L = layers[layer - 1];
        snprintf(out->name, sizeof(out->name), "%s", L.spec->name);
        if (L.kernel == kFused) {            // its MACs and bytes are accounted to the launch that runs them
            for (const Layer& C : layers)
                if (C.fused_short == layer - 1 || C.fused_next == layer - 1) snprintf(out->kernel, sizeof(out->kernel), "fused into %s", C.spec->name);
            out->flops = 0; out->min_bytes = 0; out->launches = 0;
        } else if (L.chained_into >= 0) {    // ran inside the persistent trunk launch headed by another layer (its own MACs stay its own)
            snprintf(out->kernel, sizeof(out->kernel), "chained into %s", layers[L.chained_into].spec->name);
            out->flops = L.flops; out->min_bytes = L.min_bytes; out->launches = 0;
        } else if (L.chain_len > 0) {
            snprintf(out->kernel, sizeof(out->kernel), "conv_kwave_chain_bf16 x%d", L.chain_len);
            out->flops = L.flops; out->min_bytes = L.min_bytes; out->launches = 1;
        } else {
            kernel_label(L, precision, out->kernel, sizeof(out->kernel));
            out->flops = L.flops; out->min_bytes = L.min_bytes; out->launches = 1;
            if (L.fused_next >= 0) {
                const Layer& P = layers[L.fused_next];
                out->flops += P.flops;
                out->min_bytes += P.min_bytes - 2.0 * (double)tensors[L.dst].H * tensors[L.dst].W * tensors[L.dst].Cpad * eb;
            }
            if (L.fused_short >= 0) {
                const Layer& P = layers[L.fused_short];
                out->flops += P.flops;
                // (the shortcut sums are neither written nor read: fp32 in the operand-split graph, bf16 otherwise)
                out->min_bytes += P.min_bytes - 2.0 * (double)tensors[P.dst].H * tensors[P.dst].W * tensors[P.dst].Cpad * (tensors[P.dst].is_f32 ? 4 : eb);
            }
        }
    } else if (layer == nl + 1) {
        snprintf(out->name, sizeof(out->name), "head");
        snprintf(out->kernel, sizeof(out->kernel), "head_kernel");
        out->flops = 2.0 * 128 * 2 * hw; out->min_bytes = hw * 128 * eb + hw * 2 * 4; out->launches = 1;
    } else {
        snprintf(out->name, sizeof(out->name), "dist_softmax");
        snprintf(out->kernel, sizeof(out->kernel), "softmax_nchw_kernel");
        out->launches = (flags & IDC_FLAG_DIST_HEAD) ? 1 : 0;
        out->min_bytes = out->launches ? (hw / 16) * (640 + 529) * 4 : 0;
    }
}

}  // namespace idc

extern "C" {

int idc_num_layers(idc_handle h) { return h ? h->n_timed : 0; }

int idc_layer_info_get(idc_handle h, int layer, idc_layer_info* out) {
    if (!h || !out) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null argument");
    if (layer < 0 || layer >= h->n_timed) return fail(&h->err, IDC_ERR_INVALID_ARG, "layer %d out of range", layer);
    layer_row(h->layers, h->tensors, h->precision, h->flags, h->H, h->W, layer, out);
    return IDC_OK;
}

int idc_set_range_audit(idc_handle h, int on) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (on && !h->d_audit.get()) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, h->d_audit.ensure((size_t)h->n_timed * sizeof(AuditRecord)));
        HIPCHK(h, hipMemsetAsync(h->d_audit.get(), 0, (size_t)h->n_timed * sizeof(AuditRecord), h->stream.get()));
        h->audit_values.assign((size_t)h->n_timed, 0);
    }
    h->audit = on != 0;
    return IDC_OK;
}

int idc_range_reset(idc_handle h) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (h->d_audit.get()) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemsetAsync(h->d_audit.get(), 0, (size_t)h->n_timed * sizeof(AuditRecord), h->stream.get()));     // stream-ordered behind the audited forwards
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
    if (!h->d_audit.get()) return IDC_OK;                  // never switched on: all counts zero
    HIPCHK(h, hipSetDevice(h->device));
    AuditRecord r;
    HIPCHK(h, hipMemcpyAsync(&r, h->d_audit.get() + layer, sizeof(r), hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
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
    if (on != 0) {
        HIPCHK(h, hipSetDevice(h->device));
        h->ev.resize((size_t)h->n_timed * 2 * kProfRing);
        for (auto& e : h->ev) HIPCHK(h, e.create());
    }
    h->profiling = on == 2 ? 2 : (on != 0 ? 1 : 0);
    h->prof_count = 0;
    return IDC_OK;
}

int idc_layer_times_ms(idc_handle h, float* ms, int capacity) {
    if (!h || !ms) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null argument");
    if (h->ev.empty()) return fail(&h->err, IDC_ERR_INVALID_ARG, "no forward was recorded with profiling on");
    if (capacity < h->n_timed) return fail(&h->err, IDC_ERR_INVALID_ARG, "capacity %d < %d", capacity, h->n_timed);
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    const int slots = (int)(h->prof_count < kProfRing ? h->prof_count : kProfRing);
    if (slots == 0) return fail(&h->err, IDC_ERR_INVALID_ARG, "no forward was recorded with profiling on");
    for (int i = 0; i < h->n_timed; ++i) {
        if (h->profiling == 2 && i > 0) { ms[i] = 0.f; continue; }       // mode 2: ms[0] = the whole forward
        double sum = 0;
        for (int sl = 0; sl < slots; ++sl) {
            float t = 0.f;
            const size_t base = (size_t)sl * h->n_timed * 2;
            if (hipEventElapsedTime(&t, h->ev[base + i * 2].get(), h->ev[base + i * 2 + 1].get()) != hipSuccess) { t = 0.f; (void)hipGetLastError(); }
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
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    const int slots = (int)(h->prof_count < kProfRing ? h->prof_count : kProfRing);
    if (slots == 0) return fail(&h->err, IDC_ERR_INVALID_ARG, "no forward was recorded with profiling on");
    std::vector<float> v((size_t)slots);
    for (int i = 0; i < h->n_timed; ++i) {
        if (h->profiling == 2 && i > 0) { ms_min[i] = ms_median[i] = ms_max[i] = 0.f; continue; }
        for (int sl = 0; sl < slots; ++sl) {
            float t = 0.f;
            const size_t base = (size_t)sl * h->n_timed * 2;
            if (hipEventElapsedTime(&t, h->ev[base + i * 2].get(), h->ev[base + i * 2 + 1].get()) != hipSuccess) { t = 0.f; (void)hipGetLastError(); }
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
    const int ti = find_tensor(h->tensors, name);
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
    HIPCHK(h, h->d_scratch.ensure(need * 4));
    const int src_bf16 = (!t.is_f32 && h->precision != IDC_FP32) ? 1 : 0;
    if (t.parts > 1 || (is_split(h->precision) && !t.is_f32)) HIPCHK(h, launch_split_to_nchw(      // (IDC_FP16: one fp16 plane)
        t.ptr, h->d_scratch.get(), n, t.C, t.H, t.W, t.Cpad, t.parts, split_is_f16(h->precision) ? 1 : 0, h->stream.get()));
    else HIPCHK(h, launch_nhwc_to_nchw(src_bf16, t.ptr, h->d_scratch.get(), n, t.C, t.H, t.W, t.Cpad, h->stream.get()));
    HIPCHK(h, hipMemcpyAsync(out, h->d_scratch.get(), need * 4, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
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

// One conv / deconv as a one-layer graph -- with `sc`, a two-layer graph: the 3x3 shortcut conv, whose output is the deconv's shortcut sum -- through
// the network's own plan_forward, bind_layer and launch_kernel.  What is left here: the argument checks, the graph, its parameters staged by LayerBlob
// offsets (the weight image packed once the kernel is known) and the layout conversions in and out.
static int run_single_op(int device_id, int precision, LayerSpec spec, int n, int h, int w, const float* x,
                         const float* weight, const float* bias, const float* bn_scale, const float* bn_shift,
                         const float* resid, float* y, const ShortcutOp* sc = nullptr) {
    g_op_last_kernel.clear();
    int rc = check_device(device_id, nullptr);
    if (rc) return rc;
    if (precision < IDC_FP32 || precision > IDC_FP16) return fail(nullptr, IDC_ERR_INVALID_ARG, "bad precision");
    if (!x || !weight || !bias || !y || n <= 0 || h <= 0 || w <= 0) return fail(nullptr, IDC_ERR_INVALID_ARG, "bad argument");
    const bool split = is_split(precision), f16 = split_is_f16(precision);
    const int parts = split_parts(precision);
    // operand-split precisions run the large tile only (cout >= 65) -- and, as the network runs conv1_2, its 64-cout <1,4> form on what conv1_2 is:
    // a 3x3 conv of 64 channels at dilation 1, stride 1, without a shortcut sum
    const bool tile64 = spec.kind == kConv3x3 && spec.cin == kCoutGroup && cout_pad(spec.cout) == kCoutGroup && spec.dilation == 1 && spec.in_stride == 1 && !resid;
    if (split && !v2_eligible(spec) && !tile64)
        return fail(nullptr, IDC_ERR_UNSUPPORTED, "operand-split precisions run the large tile only: cout >= 65, or a 3x3 conv (64 channels in, at most 64 out, "
                    "dilation 1, stride 1, no shortcut sum)");
    const int kc = kc_elems(precision);
    if (spec.cin % kc) return fail(nullptr, IDC_ERR_UNSUPPORTED, "cin must be a multiple of %d in this precision", kc);
    if (spec.in_stride != 1 && spec.in_stride != 2) return fail(nullptr, IDC_ERR_INVALID_ARG, "in_stride must be 1 or 2");
    if (h % spec.in_stride || w % spec.in_stride) return fail(nullptr, IDC_ERR_INVALID_ARG, "H, W must divide by in_stride");
    if (sc && (!sc->x || !sc->w || !sc->b || sc->cin <= 0 || sc->cin % kc)) return fail(nullptr, IDC_ERR_INVALID_ARG, "bad shortcut operand");
    // storage as the network's fp32-kept layers have it (options "op_out_f32", "op_resid_f32"): class / 313 logits and the hyper-column partial sums
    const bool out_f32 = options().op_out_f32 != 0, resid_f32 = options().op_resid_f32 != 0;
    if (sc && out_f32) return fail(nullptr, IDC_ERR_UNSUPPORTED, "deconv + shortcut: the fused launch stores 16-bit outputs only (option 'op_out_f32')");
    spec.out_f32 = out_f32 ? 1 : 0;          // (the planner keeps fp32-OUTPUT layers off the bf16 large tile: set_geometry's v2_covers)
    // the batch the variant is chosen for, as a handle's max_batch is (option "op_policy_batch"; 0 = this call's own batch); the launch carries n
    const int n_policy = options().op_policy_batch > 0 ? options().op_policy_batch : n;
    idc_context* nullctx = nullptr;
    HIPCHK(nullctx, hipSetDevice(device_id));
    HIPCHK(nullctx, init_kernels());
    // tensors as a network of this precision stores them: fp32 on the fp32 path, the shortcut sum bf16 on the bf16 path and fp32 on the operand-split ones;
    // "op_out_f32" / "op_resid_f32": the output / the bf16 path's shortcut sum in fp32, as a layer with LayerSpec.out_f32 stores and its consumer reads
    const int so = spec.kind == kDeconv4x4 ? 2 : 1, Ho = h / spec.in_stride * so, Wo = w / spec.in_stride * so, cpad = cout_pad(spec.cout);
    std::vector<Tensor> T;
    auto add_tensor = [&](const char* name, int C, int Cpad, int H, int W, bool f32) {
        Tensor t;
        t.name = name; t.C = C; t.Cpad = Cpad; t.H = H; t.W = W; t.is_f32 = f32; t.parts = (split && !f32) ? parts : 1;
        t.bytes = (size_t)n * H * W * Cpad * (f32 ? 4 : 2 * t.parts);
        T.push_back(t);
        return (int)T.size() - 1;
    };
    const int t_x = add_tensor("x", spec.cin, spec.cin, h, w, precision == IDC_FP32), t_y = add_tensor("y", spec.cout, cpad, Ho, Wo, precision == IDC_FP32 || out_f32);
    const int t_r = (resid || sc) ? add_tensor("resid", spec.cout, cpad, Ho, Wo, precision != IDC_BF16 || resid_f32) : -1;      // (with sc: planned, never stored)
    const int t_x2 = sc ? add_tensor("x_short", sc->cin, sc->cin, Ho, Wo, precision == IDC_FP32) : -1;
    // layers, their parameters placed in one staging blob
    size_t blob_bytes = 0;
    auto place = [&](size_t bytes) { const size_t off = blob_bytes; blob_bytes += align_up(bytes, 256); return off; };
    std::vector<Layer> layers;
    auto add_layer = [&](const LayerSpec& s, int src, int dst, int res) -> Layer& {
        Layer L;
        L.spec = &s; L.src = src; L.dst = dst; L.resid = res; L.lprec = precision; L.split = split;
        LayerBlob& lb = L.blob = LayerBlob{};
        lb.nkc = s.cin / kc; lb.ncg = cout_pad(s.cout) / kCoutGroup; lb.parts = parts;
        lb.w_bytes = (size_t)weight_taps(s.kind) * lb.nkc * lb.ncg * kWBlockBytes;
        // fp32 3x3 stride-1 ops without a shortcut sum and fp32 deconvs may take a Winograd kernel, exactly as inside the network: one slot serves either
        // image, and either layout of the direct one (the kernel decides; the packer runs after the plan)
        const bool wino = precision == IDC_FP32 && (wino_eligible(s) || wino_deconv_eligible(s));
        lb.w3_bytes = wino ? (size_t)s.cin * cout_pad(s.cout) * (s.kind == kDeconv4x4 ? 36 : 16) * 4 : 0;
        lb.w_off = lb.w2_off = place(std::max(lb.w_bytes * parts, lb.w3_bytes));
        lb.w3_off = wino ? lb.w_off : (size_t)-1;
        lb.bias_off = lb.bn_scale_off = lb.bn_shift_off = lb.fbias_off = (size_t)-1;
        fill_taps(L);
        layers.push_back(L);
        return layers.back();
    };
    // the shortcut sum arrives as a tensor; every eligibility gate of set_geometry reads spec.resid (a 3x3 op with a residual must not be handed
    // to conv_kwave_bf16 / the Winograd forms, which do not take one -- ADVICE r4)
    spec.resid = t_r >= 0 ? "resid" : nullptr;
    const LayerSpec spec2{"op_short", "op_short", nullptr, kConv3x3, sc ? sc->cin : 0, spec.cout, 1, 1, 0, "x_short", nullptr, 0, 1, 0};
    layers.reserve(2);
    if (sc) add_layer(spec2, t_x2, t_r, -1);
    Layer& op = add_layer(spec, t_x, t_y, t_r);
    op.blob.bias_off = place((size_t)cpad * 4);
    if (sc) op.blob.fbias_off = place((size_t)cpad * 4);
    if (bn_scale) { op.blob.bn_scale_off = place((size_t)cpad * 4); op.blob.bn_shift_off = place((size_t)cpad * 4); }
    if (split) op.blob.wscale_off = place(4);
    const size_t zeros_off = place(256);
    // IDC_FP16X3: the weight parts hold w * 2^e, as the blob packer does per layer; one accumulator set, one scale: the smaller exponent of a fused pair
    int op_wexp = 0;
    if (f16 && parts > 1) {
        op_wexp = f16_weight_exponent(weight, (size_t)spec.cin * spec.cout * weight_taps(spec.kind));
        if (sc) op_wexp = std::min(op_wexp, f16_weight_exponent(sc->w, (size_t)sc->cin * spec.cout * 9));
    }
    const std::vector<float> wscale(layers.size(), ldexpf(1.f, -op_wexp));
    PlanEnv pe;
    pe.precision = precision; pe.H = h; pe.W = w; pe.max_batch = n_policy; pe.n = n; pe.wscale = &wscale;
    rc = plan_forward(layers, T, pe, nullptr);
    if (rc) return rc;
    if (sc && op.fused_short < 0)
        return fail(nullptr, IDC_ERR_UNSUPPORTED, "deconv + shortcut: the network runs this pair as two launches here (policy batch %d, options)", n_policy);
    if (sc && op.kernel == kConvDs) return fail(nullptr, IDC_ERR_UNSUPPORTED, "deconv + shortcut: conv_ds_fused (the 32x32x16-MFMA partner) has no single-operator entry");
    if (op.kernel == kConv1_2Split) return fail(nullptr, IDC_ERR_UNSUPPORTED, "conv1_2_split_kernel (policy batch %d) has no single-operator entry", n_policy);
    // parameters: the weight images the chosen kernel reads, biases (padding 0), BN (padding 1, 0), the accumulator scale, the zero page
    std::vector<uint8_t> blob(blob_bytes, 0);
    auto floats = [&](size_t off) { return (float*)(blob.data() + off); };
    for (const Layer& L : layers) {
        const float* wsrc = &L == &op ? weight : sc->w;
        uint8_t* wimg = blob.data() + L.blob.w_off;
        if (L.kernel == kDeconvWino) pack_wino_deconv_weights(wimg, precision, *L.spec, L.blob, wsrc);
        else if (L.kernel == kConvWino) pack_wino_weights(wimg, precision, *L.spec, L.blob, wsrc);
        else
            for (int part = 0; part < parts; ++part)
                pack_layer_weights(wimg + (size_t)part * L.blob.w_bytes, precision, L.kernel == kConvV2 ? 2 : 1, *L.spec, L.blob, wsrc, part, ldexpf(1.f, op_wexp));
    }
    for (int c = 0; c < cpad; ++c) {
        const bool real = c < spec.cout;
        floats(op.blob.bias_off)[c] = real ? bias[c] : 0.f;
        if (sc) floats(op.blob.fbias_off)[c] = real ? bias[c] + sc->b[c] : 0.f;
        if (bn_scale) { floats(op.blob.bn_scale_off)[c] = real ? bn_scale[c] : 1.f; floats(op.blob.bn_shift_off)[c] = (real && bn_shift) ? bn_shift[c] : 0.f; }
    }
    if (split) *floats(op.blob.wscale_off) = wscale[0];
    DevMem<uint8_t> d_blob; DevMem<float> d_part, d_nchw;
    std::vector<DevMem<void>> d_t(T.size());
    HIPCHK(nullctx, d_blob.ensure(blob_bytes));
    HIPCHK(nullctx, hipMemcpy(d_blob.get(), blob.data(), blob_bytes, hipMemcpyHostToDevice));
    // fp32 NCHW on the host -> the tensor's storage on the device
    auto upload = [&](int ti, const float* src) -> int {
        Tensor& t = T[ti];
        const size_t count = (size_t)n * t.C * t.H * t.W;
        DevMem<float> raw;
        HIPCHK(nullctx, raw.ensure(count * 4));
        HIPCHK(nullctx, d_t[ti].ensure(t.bytes));
        t.ptr = d_t[ti].get();
        HIPCHK(nullctx, hipMemcpy(raw.get(), src, count * 4, hipMemcpyHostToDevice));
        if (t.parts > 1 || (split && !t.is_f32)) HIPCHK(nullctx, launch_nchw_to_split(raw.get(), t.ptr, n, t.C, t.H, t.W, t.Cpad, t.parts, f16 ? 1 : 0, nullptr));
        else HIPCHK(nullctx, launch_nchw_to_nhwc(t.is_f32 ? IDC_FP32 : IDC_BF16, raw.get(), t.ptr, n, t.C, t.H, t.W, t.Cpad, nullptr));
        HIPCHK(nullctx, hipDeviceSynchronize());          // (raw is freed on return)
        return IDC_OK;
    };
    rc = upload(t_x, x);
    if (rc == IDC_OK && resid) rc = upload(t_r, resid);
    if (rc == IDC_OK && sc) rc = upload(t_x2, sc->x);
    if (rc) return rc;
    Tensor& ty = T[t_y];
    HIPCHK(nullctx, d_t[t_y].ensure(ty.bytes));
    ty.ptr = d_t[t_y].get();
    const ConvArgs& a = op.args;
    if (a.ksplit > 1) HIPCHK(nullctx, d_part.ensure((size_t)a.ksplit * n * Ho * Wo * cpad * 4));
    BindEnv be;
    be.blob = d_blob.get(); be.tensors = &T; be.zeros = be.blob + zeros_off; be.partial = d_part.get();
    bind_layer(layers, (int)layers.size() - 1, be);
    char k[64]; kernel_label(op, precision, k, sizeof(k));
    g_op_last_kernel = k;
    if (op.kernel == kConvDsM) g_op_last_kernel += conv_ds_m_half(a) ? " half" : " 8-wave";
    const hipError_t le = launch_kernel(op.kernel, op, a, nullptr);
    if (le == hipErrorInvalidConfiguration) return fail(nullptr, IDC_ERR_INTERNAL, "single op: %s planned for a launch it does not cover", k);
    HIPCHK(nullctx, le);
    if (a.ksplit > 1) HIPCHK(nullctx, launch_splitk_epilogue(precision, a, nullptr));
    const size_t yout = (size_t)n * spec.cout * Ho * Wo;
    HIPCHK(nullctx, d_nchw.ensure(yout * 4));
    if (split && !ty.is_f32) HIPCHK(nullctx, launch_split_to_nchw(ty.ptr, d_nchw.get(), n, spec.cout, Ho, Wo, cpad, parts, f16 ? 1 : 0, nullptr));
    else HIPCHK(nullctx, launch_nhwc_to_nchw(ty.is_f32 ? 0 : 1, ty.ptr, d_nchw.get(), n, spec.cout, Ho, Wo, cpad, nullptr));
    HIPCHK(nullctx, hipMemcpy(y, d_nchw.get(), yout * 4, hipMemcpyDeviceToHost));
    HIPCHK(nullctx, hipDeviceSynchronize());
    return IDC_OK;
}

int idc_op_conv2d(int device_id, int precision, int n, int cin, int h, int w, const float* x, int cout, int ksize,
                  int dilation, int in_stride, const float* weight, const float* bias, int act, const float* bn_scale,
                  const float* bn_shift, const float* resid, float* y) {
    if (ksize != 3 && ksize != 1) return fail(nullptr, IDC_ERR_UNSUPPORTED, "ksize must be 1 or 3");
    if (dilation != 1 && dilation != 2) return fail(nullptr, IDC_ERR_UNSUPPORTED, "dilation must be 1 or 2");
    if (ksize == 1 && (dilation != 1 || in_stride != 1)) return fail(nullptr, IDC_ERR_UNSUPPORTED, "1x1 conv: d=1, stride 1 only");
    // (out_f32 = 0 in the three specs below; run_single_op sets it from option "op_out_f32", with the output tensor's storage)
    LayerSpec s{"op", "op", nullptr, ksize == 3 ? kConv3x3 : kConv1x1, cin, cout, dilation, in_stride, act,
                "x", nullptr, 0, 1, 0};
    return run_single_op(device_id, precision, s, n, h, w, x, weight, bias, bn_scale, bn_shift, resid, y);
}

int idc_op_last_kernel(char* out, int cap) {
    if (!out || cap <= 0) return fail(nullptr, IDC_ERR_INVALID_ARG, "null / empty label buffer");
    snprintf(out, (size_t)cap, "%s", g_op_last_kernel.c_str());
    return IDC_OK;
}

int idc_grid_last(const char* tag, long long* want, int* blocks) {
    const int i = grid_tag_index(tag);
    if (i < 0) return fail(nullptr, IDC_ERR_INVALID_ARG, "unknown grid tag '%s'", tag ? tag : "(null)");
    const GridRecord r = grid_last(i);
    if (want) *want = r.want;
    if (blocks) *blocks = r.blocks;
    return IDC_OK;
}

const char* idc_grid_tag(int i) { return grid_tag_name(i); }

int idc_op_deconv_shortcut(int device_id, int precision, int n, int cin, int h, int w, const float* x, int cout, const float* w_deconv,
                           const float* b_deconv, int cin_short, const float* x_short, const float* w_short, const float* b_short, int act, float* y) {
    LayerSpec s{"op", "op", nullptr, kDeconv4x4, cin, cout, 1, 1, act, "x", nullptr, 0, 1, 0};
    const ShortcutOp sc{cin_short, x_short, w_short, b_short};
    return run_single_op(device_id, precision, s, n, h, w, x, w_deconv, b_deconv, nullptr, nullptr, nullptr, y, &sc);
}

int idc_op_deconv4x4s2(int device_id, int precision, int n, int cin, int h, int w, const float* x, int cout,
                       const float* weight, const float* bias, int act, const float* resid, float* y) {
    LayerSpec s{"op", "op", nullptr, kDeconv4x4, cin, cout, 1, 1, act, "x", nullptr, 0, 1, 0};
    return run_single_op(device_id, precision, s, n, h, w, x, weight, bias, nullptr, nullptr, resid, y);
}

}  // extern "C"
