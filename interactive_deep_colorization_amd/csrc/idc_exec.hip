// idc_exec.hip -- the executor: one forward of the graph on the handle's stream (run_graph: plan_forward, then bind_layer and a launch per layer, or the persistent kwave chain), the host-pointer
// forward with its transfers, the two-slot transfer pipeline, and the forward entry points of the C ABI (include/ideepcolor.h).
// Replaces: SIGGRAPHGenerator.forward (models/pytorch/model.py:6-175).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "idc_engine.h"

namespace idc {

// The run of same-shape 8-chunk conv_kwave_bf16 layers that starts at layer li (conv4_2 .. conv7_3 at batch 1) as ONE persistent
// conv_kwave_chain_bf16 launch, where the handle and the device allow it: on success L.chain_len > 0 and *chain_until = the run's last
// layer; otherwise nothing is launched and the caller launches layer li alone.
static int launch_kwave_chain(idc_context* c, int li, hipStream_t s, int* chain_until) {
    Layer& L = c->layers[li];
    const ConvArgs& a = L.args;
    if (!options().kwave_chain || c->kw_chain_off || c->profiling == 1 || !c->d_kw_bar.get() || L.spec->kind != kConv3x3 || a.nkc != 8 || a.si != 1 ||
        a.img_shift != nullptr || a.out_f32)
        return IDC_OK;
    const int blocks = conv_kwave_chain_blocks(a.Hs, a.Ws, a.N, a.ncg, a.dy[8]);
    KwChainArgs ch{};
    ch.H = a.Hs; ch.W = a.Ws; ch.N = a.N; ch.ncg = a.ncg;
    ch.spin_limit = 200000u;                   // x ~1.5 us per poll: a third of a second, then the workgroup gives up
    int last = li, prev_dst = L.src;
    for (int j = li; j < (int)c->layers.size() && ch.nlayers < kKwChainMax; ++j) {
        Layer& Q = c->layers[j];
        if (Q.kernel != kConvKwave || Q.spec->kind != kConv3x3 || Q.blob.nkc != 8 || Q.spec->in_stride != 1 || Q.resid >= 0 || Q.shifted ||
            c->tensors[Q.dst].is_f32 || Q.src != prev_dst || Q.args.Hs != a.Hs || Q.args.Ws != a.Ws || Q.args.ncg != a.ncg ||
            conv_kwave_chain_blocks(a.Hs, a.Ws, a.N, a.ncg, Q.args.dy[8]) != blocks)
            break;
        KwChainLayer& y = ch.layer[ch.nlayers++];
        y.in = c->tensors[Q.src].ptr; y.out = c->tensors[Q.dst].ptr;
        y.wgt = c->d_blob + Q.blob.w_off;
        y.bias = (const float*)(c->d_blob + Q.blob.bias_off);
        y.bn_scale = Q.blob.bn_scale_off != (size_t)-1 ? (const float*)(c->d_blob + Q.blob.bn_scale_off) : nullptr;
        y.bn_shift = Q.blob.bn_shift_off != (size_t)-1 ? (const float*)(c->d_blob + Q.blob.bn_shift_off) : nullptr;
        y.act = Q.spec->act; y.d = Q.args.dy[8];
        prev_dst = Q.dst; last = j;
    }
    if (ch.nlayers < 2 || blocks <= 0) return IDC_OK;
    if (c->kw_chain_fits < 0) c->kw_chain_fits = conv_kwave_chain_capacity(c->device);
    if (c->kw_chain_fits < blocks) return IDC_OK;   // more workgroups than the chip holds at once: this launch goes layer by layer
    if (blocks != c->kw_bar_blocks) {      // counters hold (barriers so far) x (arrivals per barrier of THIS grid)
        HIPCHK(c, hipMemsetAsync(c->d_kw_bar.get(), 0, 1024, s));
        c->kw_bar_count = 0; c->kw_bar_blocks = blocks;
    }
    ch.bar = c->d_kw_bar.get(); ch.bar_base = c->kw_bar_count; ch.abort_flag = c->h_kw_abort.get();
    // test hook (tests/test_round5_gpu.py): IDC_KW_FORCE_ABORT=1 makes the first grid barrier unreachable and the give-up
    // counter tiny, i.e. it plays "the workgroups never become co-resident" on a healthy device
    if (options().kw_force_abort) { ch.bar_base += 1000; ch.spin_limit = 20u; }
    static const bool want_stamps = idc_env_int("IDC_KW_STAMPS", 0) != 0;
    if (want_stamps) HIPCHK(c, c->d_kw_stamps.ensure((size_t)4096 * kKwChainMax * 8 * 8));
    ch.stamps = (want_stamps && blocks <= 4096) ? c->d_kw_stamps.get() : nullptr;
    c->kw_stamp_layers = ch.nlayers; c->kw_stamp_blocks = blocks;
    if (launch_conv_kwave_chain(ch, blocks, options().kwave_chain, s) != hipSuccess) {
        (void)hipGetLastError();          // refused (e.g. hipErrorCooperativeLaunchTooLarge): one launch per layer from now on
        c->kw_chain_off = true;
        return IDC_OK;
    }
    c->kw_bar_count += (unsigned long long)(ch.nlayers - 1);
    L.chain_len = ch.nlayers;
    for (int j = li + 1; j <= last; ++j) c->layers[j].chained_into = li;
    *chain_until = last;
    return IDC_OK;
}

// A planned layer's pointers: this forward's tensors, the layer's parameters in the blob (the weight image the chosen kernel reads) and what rides
// in the launch.  Decides nothing: which kernel runs, with which geometry and which optional operands, is the plan's (plan_forward, whose
// args_as_bound states the same operands without the pointers).
void bind_layer(std::vector<Layer>& layers, int li, const BindEnv& e) {
    Layer& L = layers[li];
    ConvArgs& a = L.args;
    const std::vector<Tensor>& T = *e.tensors;
    auto at = [&](size_t off) -> const float* { return off != (size_t)-1 ? (const float*)(e.blob + off) : nullptr; };
    const Layer* S = L.fused_short >= 0 ? &layers[L.fused_short] : nullptr;      // the shortcut conv in this launch's K loop (model.py:156,170,172)
    const Layer* P = L.fused_next >= 0 ? &layers[L.fused_next] : nullptr;        // conv1_2 in conv1_1's launch (launch_conv1_block's argument convention)
    const bool wino = L.kernel == kConvWino || L.kernel == kDeconvWino, lay2 = L.kernel == kConvV2 || L.kernel == kConvDs;
    a.in = T[L.src].ptr;
    a.out = T[P ? P->dst : L.dst].ptr;
    a.wgt = e.blob + (lay2 && L.blob.w2_off != (size_t)-1 ? L.blob.w2_off : wino ? L.blob.w3_off :
                      (P && a.split_f16) ? L.blob.w2_off : L.blob.w_off);        // (IDC_FP16 model1: conv1_1's fp16 block, conv1_block_fused_th)
    a.bias = at(S ? L.blob.fbias_off : L.blob.bias_off);
    a.bn_scale = at(P ? P->blob.bn_scale_off : L.blob.bn_scale_off);
    a.bn_shift = at(P ? P->blob.bn_shift_off : L.blob.bn_shift_off);
    a.resid = (!S && L.resid >= 0) ? T[L.resid].ptr : nullptr;
    a.img_shift = L.shifted ? e.glob_vec : nullptr;
    a.in2 = S ? T[S->src].ptr : nullptr;
    a.wgt2 = S ? e.blob + (L.kernel == kConvDs && S->blob.w2_off != (size_t)-1 ? S->blob.w2_off : S->blob.w_off) : P ? e.blob + P->blob.w_off : nullptr;
    if (L.spec->kind == kConvIm2col) {          // model.py:139-148 input pack, fused into the operand staging
        a.pk_L = e.L; a.pk_ab = e.ab; a.pk_mask = e.mask;
        a.pk_ldiv = e.l_div; a.pk_abdiv = e.ab_div; a.pk_mmul = e.mask_mul; a.pk_mcent = e.mask_cent;
    } else {
        a.pk_L = nullptr;
    }
    a.head_w = L.fused_head ? at(e.head_w_off) : nullptr;
    a.head_b = P ? at(P->blob.bias_off) : at(e.head_b_off);
    a.head_out = e.out; a.head_mul = e.out_mul;
    a.acc_scale = (L.split && a.split_f16) ? at(L.blob.wscale_off) : nullptr;
    a.zeros = e.zeros;
    a.partial = a.ksplit > 1 ? e.partial : nullptr;
}

int run_graph(idc_context* c, int n, const float* dL, const float* dab, const float* dmask, float maskcent,
                     float* dout, float* ddist, const float* glob_in) {
    hipStream_t s = c->stream.get();
    int step = 0;
    {   // a workgroup of an EARLIER conv_kwave_chain_bf16 launch gave up at its grid barrier and nobody has waited on that forward since
        const int arc = check_chain_abort(c);
        if (arc) return arc;
    }
    const size_t ring = (size_t)(c->prof_count % kProfRing) * c->n_timed * 2;
    auto tic = [&]() { if (c->profiling == 1) (void)hipEventRecord(c->ev[ring + step * 2].get(), s); };
    auto toc = [&]() { if (c->profiling == 1) (void)hipEventRecord(c->ev[ring + step * 2 + 1].get(), s); ++step; };
    // range audit: the stored output of layer index lj, folded into its record right behind the launch that wrote it (outside the event pairs)
    auto audit_layer = [&](int lj) -> hipError_t {
        const Layer& Q = c->layers[lj];
        const Tensor& t = c->tensors[Q.dst];
        const int parts = t.is_f32 ? 0 : t.parts;
        c->audit_values[lj + 1] += (unsigned long long)n * t.C * t.H * t.W;
        return launch_range_audit(t.ptr, (long long)n * t.H * t.W, t.C, t.Cpad, parts, split_is_f16(c->precision) ? 1 : 0, c->d_audit.get() + lj + 1, s);
    };
    if (c->profiling == 2) (void)hipEventRecord(c->ev[ring].get(), s);          // whole-forward pair: slot 0
    tic();   // (slot 0: the input pack is fused into conv1_1's operand staging; only the global-hints branch runs here)
    if (c->flags & IDC_FLAG_GLOBAL_HINTS)      // four GEMVs per image; its output is consumed by conv4_3's epilogue
        HIPCHK(c, launch_glob_branch(glob_in, (const float*)(c->d_blob + c->plan.glob_off), c->d_glob_vec.get(), n, s));
    toc();
    PlanEnv pe;
    pe.precision = c->precision; pe.flags = c->flags; pe.H = c->H; pe.W = c->W; pe.max_batch = c->max_batch; pe.n = n;
    pe.t_conv10_2 = c->t_conv10_2; pe.t_conv4_3 = c->t_conv4_3; pe.wscale = &c->wscale;
    const int prc = plan_forward(c->layers, c->tensors, pe, &c->err);
    if (prc) return prc;
    BindEnv be;
    be.blob = c->d_blob; be.head_w_off = c->plan.head_w_off; be.head_b_off = c->plan.head_b_off;
    be.tensors = &c->tensors; be.zeros = c->d_zeros.get(); be.glob_vec = c->d_glob_vec.get();
    be.L = dL; be.ab = dab; be.mask = dmask; be.l_div = c->l_div; be.ab_div = c->ab_div; be.mask_mul = c->mask_mul; be.mask_cent = maskcent;
    be.out = dout; be.out_mul = c->out_mul;
    // diagnostic (IDC_DOUBLE_LAUNCH=1): every launch issued twice, the event pair around the SECOND -- a layer that is slow only as
    // the first launch of its kernel after other kernels (cold instruction cache / first touch) shows its warm time here
    static const bool double_launch = idc_env_int("IDC_DOUBLE_LAUNCH", 0) != 0;
    bool head_done = false;
    int chain_until = -1;                      // layers up to this index ran inside the conv_kwave_chain_bf16 launch of an earlier layer
    for (int li = 0; li < (int)c->layers.size(); ++li) {
        Layer& L = c->layers[li];
        const Tensor& to = c->tensors[L.dst];
        const ConvArgs& a = L.args;
        L.chain_len = 0;
        if (li > chain_until) L.chained_into = -1;
        if (L.kernel == kFused || li <= chain_until) { tic(); toc(); continue; }
        if (a.ksplit > 1) {
            const size_t need = (size_t)a.ksplit * n * to.H * to.W * to.Cpad * 4;
            if (c->d_partial.bytes() < need) {
                HIPCHK(c, hipStreamSynchronize(s));
                HIPCHK(c, c->d_partial.ensure(need));
            }
        }
        be.partial = c->d_partial.get();
        bind_layer(c->layers, li, be);
        head_done = head_done || L.fused_head;
        for (int rep = double_launch ? 0 : 1; rep < 2; ++rep) {
            if (rep == 1) tic();
            bool chained = false;
            if (L.kernel == kConvKwave && !double_launch) {
                const int rc = launch_kwave_chain(c, li, s, &chain_until);
                if (rc) return rc;
                chained = L.chain_len > 0;
            }
            const hipError_t le = chained ? hipSuccess : launch_kernel(L.kernel, L, a, s);
            if (le == hipErrorInvalidConfiguration) {
                char k[64]; kernel_label(L, c->precision, k, sizeof(k));
                return fail(&c->err, IDC_ERR_INTERNAL, "layer %s: %s planned for a launch it does not cover%s", L.spec->name, k,
                            kAbPartners ? "" : " (the default library has no conv_igemm_v2 / conv_ds_fused / conv1_1_bf16_kernel: -DIDC_AB_PARTNERS)");
            }
            HIPCHK(c, le);
            if (a.ksplit > 1) HIPCHK(c, launch_splitk_epilogue(L.lprec, a, s));
        }
        toc();
        if (c->audit) {
            if (L.fused_next >= 0) HIPCHK(c, audit_layer(L.fused_next));              // model1 in one launch: conv1_2's output is what was stored
            else if (L.chain_len > 0) { for (int j = li; j <= chain_until; ++j) HIPCHK(c, audit_layer(j)); }
            else if (!L.fused_head) HIPCHK(c, audit_layer(li));                      // (conv10_2 under the fused head: never stored)
        }
    }
    tic();
    if (!head_done && is_split(c->precision))
        return fail(&c->err, IDC_ERR_INTERNAL, "operand-split forward: the regression head did not ride in conv10_2's launch");
    if (!head_done)
        HIPCHK(c, launch_head(c->precision, c->tensors[c->t_conv10_2].ptr, (const float*)(c->d_blob + c->plan.head_w_off),
                              (const float*)(c->d_blob + c->plan.head_b_off), dout, n, c->H, c->W, c->out_mul, s));
    toc();
    tic();
    if (ddist) {
        const Tensor& tl = c->tensors[c->t_logits];
        HIPCHK(c, launch_softmax_nchw((const float*)tl.ptr, ddist, n, tl.H, tl.W, 529, tl.Cpad, 0.2f, s));
    }
    if (c->flags & IDC_FLAG_DIST313) {         // bilinear x4 + softmax(S.) + softmax(2.6 .) -> pred_ab decode
        const Tensor& tp = c->tensors[c->t_pred313];
        HIPCHK(c, launch_dist313((const float*)tp.ptr, (const float*)(c->d_blob + c->plan.pred_ab_off), c->d_pred_ab.get(),
                                 (c->want_dist313 || c->keep_dist313) ? c->d_dist313.get() : nullptr, n, c->H, c->W, tp.Cpad,
                                 c->dist_S, 2.6f, s));
    }
    toc();
    c->dist_n = (ddist || ((c->flags & IDC_FLAG_DIST313) && (c->want_dist313 || c->keep_dist313))) ? n : 0;
    if (dout == c->d_out.get()) c->last_n = n;       // images whose ab map sits in the handle's own d_out (display step source)
    if (c->profiling == 2) (void)hipEventRecord(c->ev[ring + 1].get(), s);
    if (c->profiling) ++c->prof_count;
    return IDC_OK;
}

// A conv_kwave_chain_bf16 workgroup that gave up at its grid barrier (not all workgroups co-resident: a partitioned or shared device) set the pinned
// flag: the results of the forward that has just been waited for are invalid.  Called after the synchronising points of the blocking entry points.
int check_chain_abort(idc_context* c) {
    if (c->h_kw_abort.get() && *c->h_kw_abort.get()) {
        *c->h_kw_abort.get() = 0;
        c->kw_chain_off = true;
        return fail(&c->err, IDC_ERR_INTERNAL, "the persistent trunk launch (conv_kwave_chain_bf16) did not get all its workgroups co-resident and timed "
                    "out: this forward's result is invalid; the handle now runs one launch per layer -- call again");
    }
    return IDC_OK;
}

int check_forward_args(idc_context* c, int n) {
    if (!c) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!c->weights_set) return fail(&c->err, IDC_ERR_NO_WEIGHTS, "I need to have a net! (no weights loaded)");
    if (n <= 0 || n > c->max_batch) return fail(&c->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, c->max_batch);
    return IDC_OK;
}

// The end of a click: hipStreamSynchronize parks the thread on an interrupt (tens of microseconds to come back, against a 0.3-1.1 ms forward); the calls
// that serve ONE OR TWO images poll the stream instead (bounded: after ~4 ms of polling -- several forwards -- it blocks like everybody else).  Batches
// keep the blocking wait: there the CPU is better spent elsewhere.  IDC_SPIN_SYNC=0 restores the blocking wait everywhere (A/B).
hipError_t wait_stream(idc_context* c, int n) {
    const bool spin = options().spin_sync != 0;
    if (spin && n <= 2) {
        for (int i = 0; i < 4000; ++i) {
            const hipError_t e = hipStreamQuery(c->stream.get());
            if (e != hipErrorNotReady) return e;
#if defined(__x86_64__) || defined(__i386__)
            for (int k = 0; k < 40; ++k) __builtin_ia32_pause();
#else
            for (volatile int k = 0; k < 40; ++k) {}
#endif
        }
    }
    return hipStreamSynchronize(c->stream.get());
}

// A click's transfers (<= 2 MiB between pinned host memory and HBM) run as a kernel on the forward's stream (pcie_copy_kernel, idc_kernels.hip) instead of
// going to a copy engine: no cross-queue hand-over on either side of them.  `host` must be pinned (ours, or the caller's idc_alloc_host / hipHostMalloc /
// mapped hipHostRegister memory); anything the device cannot address, bigger, or not 16-byte shaped takes hipMemcpyAsync.  IDC_PCIE_KERNEL=0: always (A/B).
hipError_t copy_h2d_or_d2h(idc_context* c, void* dev, void* host, size_t bytes, bool to_device) {
    const bool by_kernel = options().pcie_kernel != 0;
    if (by_kernel && bytes <= ((size_t)2 << 20) && bytes % 16 == 0 && (((uintptr_t)dev | (uintptr_t)host) & 15) == 0) {
        void* hv = nullptr;
        if (hipHostGetDevicePointer(&hv, host, 0) == hipSuccess && hv)
            return to_device ? launch_pcie_copy(dev, hv, bytes, c->stream.get()) : launch_pcie_copy(hv, dev, bytes, c->stream.get());
        (void)hipGetLastError();
    }
    return to_device ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream.get()) : hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream.get());
}

// finish = false: everything is enqueued (the D2H of the ab map into h_out included) but the stream is NOT synchronised and
// nothing is copied to out_ab -- idc_forward_rgb appends the colour step and synchronises once for both
static int forward_host(idc_context* c, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                        float* out_ab, float* dist_q, bool keep_dist = false, bool finish = true, bool copy_out = true) {
    int rc = check_forward_args(c, n);
    if (rc) return rc;
    if (!ab || !mask || (copy_out && !out_ab)) return fail(&c->err, IDC_ERR_INVALID_ARG, "null tensor pointer");
    if (!L_mc) {                             // L_mc == NULL: the L planes idc_set_image_l left in the handle (constant between the clicks on one image)
        if (copy_out) return fail(&c->err, IDC_ERR_INVALID_ARG, "null tensor pointer");      // (only idc_forward_rgb_lazy offers this form)
        for (int i = 0; i < n; ++i)
            if (!c->l_set[i]) return fail(&c->err, IDC_ERR_INVALID_ARG, "L_mc is NULL and image %d has no resident L plane (idc_set_image_l)", i);
    }
    if ((dist_q || keep_dist) && !(c->flags & IDC_FLAG_DIST_HEAD))
        return fail(&c->err, IDC_ERR_UNSUPPORTED, "handle was created without IDC_FLAG_DIST_HEAD");
    HIPCHK(c, hipSetDevice(c->device));
    rc = drain_pipeline(c);
    if (rc) return rc;
    const size_t hw = (size_t)c->H * c->W;
    if (L_mc) for (int i = 0; i < n; ++i) { c->l_set[i] = 1; drop_source(c, i); }
    c->out_resident = true; c->labq_resident = false;
    // Pinned caller buffers (idc_alloc_host / hipHostMalloc / hipHostRegister) are transferred in place; pageable ones go through
    // the handle's pinned staging with a host memcpy (2.2 MB per click through the reference API: most of its host-side time).
    // Staged in pieces (>= 256 KiB, at most four per tensor), each piece's DMA issued as soon as it is in the staging buffer: the copy engine moves piece k
    // while the CPU copies piece k + 1, so a click pays the host memcpy plus ONE piece of DMA instead of memcpy + all of it.
    float* hL = c->h_in.get(); float* hab = hL + (size_t)n * hw; float* hm = hab + (size_t)n * hw * 2;
    auto upload = [&](void* dst, const float* src, float* staging, size_t bytes) -> hipError_t {
        if (is_pinned(src)) return copy_h2d_or_d2h(c, dst, (void*)src, bytes, true);
        size_t piece = (bytes + 3) / 4;
        if (piece < (size_t)256 * 1024) piece = (size_t)256 * 1024;
        piece = (piece + 4095) & ~(size_t)4095;
        for (size_t o = 0; o < bytes; o += piece) {
            const size_t m = bytes - o < piece ? bytes - o : piece;
            memcpy((char*)staging + o, (const char*)src + o, m);
            const hipError_t e = copy_h2d_or_d2h(c, (char*)dst + o, (char*)staging + o, m, true);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    if (L_mc) HIPCHK(c, upload(c->d_L.get(), L_mc, hL, (size_t)n * hw * 4));
    HIPCHK(c, upload(c->d_ab.get(), ab, hab, (size_t)n * hw * 2 * 4));
    HIPCHK(c, upload(c->d_mask.get(), mask, hm, (size_t)n * hw * 4));
    rc = run_graph(c, n, c->d_L.get(), c->d_ab.get(), c->d_mask.get(), maskcent, c->d_out.get(), (dist_q || keep_dist) ? c->d_dist.get() : nullptr, c->d_glob_in.get());
    if (rc) return rc;
    const bool out_direct = copy_out && out_ab != c->h_out.get() && is_pinned(out_ab);
    c->out_copy_pending = copy_out && out_ab != c->h_out.get() && !out_direct;
    if (copy_out)          // (copy_out = false: the ab map stays in d_out -- idc_fetch_outputs brings it over when somebody asks)
        HIPCHK(c, copy_h2d_or_d2h(c, c->d_out.get(), out_direct ? out_ab : c->h_out.get(), (size_t)n * hw * 2 * 4, false));
    const size_t dq = (size_t)n * 529 * (hw / 16) * 4;
    if (dist_q) HIPCHK(c, hipMemcpyAsync(c->h_dist.get(), c->d_dist.get(), dq, hipMemcpyDeviceToHost, c->stream.get()));
    if (!finish) return IDC_OK;
    HIPCHK(c, wait_stream(c, n));
    rc = check_chain_abort(c);
    if (rc) return rc;
    if (c->out_copy_pending) memcpy(out_ab, c->h_out.get(), (size_t)n * hw * 2 * 4);
    c->out_copy_pending = false;
    if (dist_q) memcpy(dist_q, c->h_dist.get(), dq);
    return IDC_OK;
}

bool is_pinned(const void* p) {
    hipPointerAttribute_t at;
    const hipError_t e = hipPointerGetAttributes(&at, p);
    (void)hipGetLastError();                      // pageable memory is "invalid value" to this query: not an error of ours, never sticky
    return e == hipSuccess && at.type == hipMemoryTypeHost;
}

static int ensure_pipeline(idc_context* h) {
    const size_t hw = (size_t)h->H * h->W, nb = (size_t)h->max_batch;
    HIPCHK(h, h->s_in.create(hipStreamNonBlocking));
    HIPCHK(h, h->s_out.create(hipStreamNonBlocking));
    for (auto& sl : h->pipe) {
        // both slots own their planes (50 MB each at N = 32): nothing here aliases the handle's resident L / hint / output
        // planes, so the copy-in stream never has to be ordered against the compute stream (ordering slot 0's copies behind
        // "everything enqueued so far" serialises them behind the OTHER slot's kernels: measured 0.89 instead of 0.97 of
        // the device-resident rate, profiles/r03a_bench.json)
        HIPCHK(h, sl.d_L.ensure(nb * hw * 4));
        HIPCHK(h, sl.d_ab.ensure(nb * hw * 2 * 4));
        HIPCHK(h, sl.d_mask.ensure(nb * hw * 4));
        HIPCHK(h, sl.d_out.ensure(nb * hw * 2 * 4));
        // timing-capable events: idc_pipeline_times reports where each stage of a batch sat on the device's clock
        Event* evs[] = {&sl.ev_in, &sl.ev_comp, &sl.ev_out, &sl.ev_in0, &sl.ev_comp0, &sl.ev_out0};
        for (Event* e : evs) HIPCHK(h, e->create());
    }
    HIPCHK(h, h->ev_pipe_base.create());
    if (!h->pipe_ready) HIPCHK(h, hipEventRecord(h->ev_pipe_base.get(), h->stream.get()));
    h->pipe_ready = true;
    return IDC_OK;
}

static int wait_slot(idc_context* h, int slot) {
    auto& sl = h->pipe[slot];
    if (!sl.pending) return IDC_OK;
    HIPCHK(h, hipEventSynchronize(sl.ev_out.get()));
    sl.pending = false;
    const int arc = check_chain_abort(h);      // the forward this slot carried ran a chain launch that gave up: its result is invalid
    if (arc) return arc;
    for (const auto& o : sl.outs) memcpy(o.user, o.pinned, o.bytes);
    return IDC_OK;
}

// `bytes` at `at` of a slot's device block to the caller's buffer, on the copy-out stream: in place when the buffer is pinned (direct), else
// into the block's pinned twin at the same offset, where it waits for idc_wait (sl.outs)
static hipError_t copy_out(idc_context* h, idc_context::PipeSlot& sl, void* user, bool direct, const void* dev, void* twin, size_t at, size_t bytes) {
    void* dst = direct ? user : (void*)((unsigned char*)twin + at);
    const hipError_t e = hipMemcpyAsync(dst, (const unsigned char*)dev + at, bytes, hipMemcpyDeviceToHost, h->s_out.get());
    if (e == hipSuccess && !direct) sl.outs.push_back({user, dst, bytes});
    return e;
}

int drain_pipeline(idc_context* c) {
    if (!c->pipe_ready) return IDC_OK;
    for (int k = 0; k < 2; ++k) { int rc = wait_slot(c, k); if (rc) return rc; }
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- reference-image global hints
int check_refs(idc_context* c, int m_min, int n, int m, const idc_ref_image* refs, const int32_t* ref_index, const float* centres,
               float hist_flag, unsigned ref_flags, RefLayout* lay) {
    if (m < m_min || m > IDC_REF_MAX) return fail(&c->err, IDC_ERR_INVALID_ARG, "%d references outside %d..%d", m, m_min, IDC_REF_MAX);
    if (m > 0 && !refs) return fail(&c->err, IDC_ERR_INVALID_ARG, "null refs");
    if (m > 0 && !centres) return fail(&c->err, IDC_ERR_INVALID_ARG, "null centres");
    if (ref_flags & ~(unsigned)IDC_REF_SATURATION) return fail(&c->err, IDC_ERR_INVALID_ARG, "unknown reference flag bits 0x%x", ref_flags);
    if (!std::isfinite(hist_flag)) return fail(&c->err, IDC_ERR_INVALID_ARG, "hist_flag is not finite");
    size_t bytes = 0;
    for (int r = 0; r < m; ++r) {
        if (!refs[r].rgb) return fail(&c->err, IDC_ERR_INVALID_ARG, "reference %d: null rgb", r);
        if (refs[r].h < 1 || refs[r].h > 16384 || refs[r].w < 1 || refs[r].w > 16384)
            return fail(&c->err, IDC_ERR_INVALID_ARG, "reference %d: size %dx%d outside 1..16384", r, refs[r].h, refs[r].w);
        bytes += (size_t)refs[r].h * refs[r].w * 3;               // <= 4096 * 0.8 GB: no overflow in 64 bits
    }
    if (bytes > IDC_BATCH_MAX_SOURCE_BYTES)
        return fail(&c->err, IDC_ERR_INVALID_ARG, "%d references hold %zu bytes, more than %zu", m, bytes, (size_t)IDC_BATCH_MAX_SOURCE_BYTES);
    if (n > 0 && m > 0) {
        if (!ref_index && m != n) return fail(&c->err, IDC_ERR_INVALID_ARG, "null ref_index needs m == n (m = %d, n = %d)", m, n);
    }
    if (n > 0 && ref_index)
        for (int i = 0; i < n; ++i)
            if (ref_index[i] < -1 || ref_index[i] >= m) return fail(&c->err, IDC_ERR_INVALID_ARG, "ref_index[%d] = %d outside -1..%d", i, ref_index[i], m - 1);
    const size_t mm = m > 0 ? (size_t)m : 1, nn = n > 0 ? (size_t)n : 1, G = (size_t)ref_stats_workgroups(c->H, c->W);
    lay->n = n; lay->m = m; lay->ref_bytes = bytes;
    lay->o_index = align_up(mm * sizeof(RefDesc), 16);
    lay->o_centres = lay->o_index + align_up(nn * sizeof(int), 16);
    lay->o_packed = lay->o_centres + align_up(626 * sizeof(float), 16);
    lay->in_bytes = lay->o_packed + bytes;
    lay->up_bytes = lay->dev_bytes = lay->in_bytes;
    if (c->ingest_filter == IDC_FILTER_ANTIALIAS)         // the handle's setting as it is now; a reference no larger than the net keeps today's rule
        for (int r = 0; r < m; ++r) {
            if (!resample_applies(refs[r].h, refs[r].w, c->H, c->W)) continue;
            const int tiles = resample_tile_count(c->W, resample_tile_width(refs[r].w, c->W, 3));
            lay->aa_tiles = lay->aa_tiles > tiles ? lay->aa_tiles : tiles;
            ++lay->naa;
        }
    if (lay->naa > 0) {
        lay->o_jobs = align_up(lay->in_bytes, 16);
        lay->up_bytes = lay->o_jobs + (size_t)lay->naa * sizeof(ResampleJob);
        lay->o_aa = align_up(lay->up_bytes, 16);
        lay->dev_bytes = lay->o_aa + (size_t)lay->naa * c->H * c->W * 3;
    }
    lay->o_sat = align_up(mm * 313 * sizeof(unsigned), 16);
    lay->o_hist = lay->o_sat + align_up(mm * G * sizeof(double), 16);
    lay->o_savg = lay->o_hist + align_up(mm * 313 * sizeof(float), 16);
    lay->work_bytes = lay->o_savg + align_up(mm * sizeof(float), 16);
    return IDC_OK;
}

int stage_refs(idc_context* c, idc_context::RefStage& st, const RefLayout& lay, const idc_ref_image* refs, const int32_t* ref_index,
               const float* centres, bool want_results) {
    HIPCHK(c, st.h_in.ensure(lay.up_bytes, 65536));
    HIPCHK(c, st.d_in.ensure(lay.dev_bytes, 65536));
    HIPCHK(c, st.d_work.ensure(lay.work_bytes, 65536));
    if (want_results) HIPCHK(c, st.h_res.ensure(lay.work_bytes - lay.o_hist, 65536));
    unsigned char* base = st.h_in.get();
    RefDesc* tab = (RefDesc*)base;
    ResampleJob* jobs = (ResampleJob*)(base + lay.o_jobs);
    const size_t net_bytes = (size_t)c->H * c->W * 3;
    size_t off = 0;
    for (int r = 0, k = 0; r < lay.m; ++r) {
        const size_t sb = (size_t)refs[r].h * refs[r].w * 3;
        tab[r].off = (long long)off; tab[r].h = refs[r].h; tab[r].w = refs[r].w;
        memcpy(base + lay.o_packed + off, refs[r].rgb, sb);
        if (lay.naa > 0 && resample_applies(refs[r].h, refs[r].w, c->H, c->W)) {   // the statistics read the net-size image the pre-pass makes of it
            const size_t dst = lay.o_aa + (size_t)k * net_bytes;
            jobs[k++] = resample_job((long long)(lay.o_packed + off), (long long)dst, refs[r].h, refs[r].w, c->W, 3);
            tab[r].off = (long long)dst - (long long)lay.o_packed; tab[r].h = c->H; tab[r].w = c->W;
        }
        off += sb;
    }
    int* idx = (int*)(base + lay.o_index);
    for (int i = 0; i < lay.n; ++i) idx[i] = lay.m == 0 ? -1 : (ref_index ? ref_index[i] : i);
    if (lay.m > 0) memcpy(base + lay.o_centres, centres, 626 * sizeof(float));
    return IDC_OK;
}

int upload_refs(idc_context* c, idc_context::RefStage& st, const RefLayout& lay, hipStream_t copy) {
    // without references only the index travels (every entry -1): the table, the centres and the packed section are not read
    const size_t bytes = lay.m > 0 ? lay.up_bytes : lay.o_centres;
    HIPCHK(c, hipMemcpyAsync(st.d_in.get(), st.h_in.get(), bytes, hipMemcpyHostToDevice, copy));
    return IDC_OK;
}

int launch_refs(idc_context* c, idc_context::RefStage& st, const RefLayout& lay, float hist_flag, unsigned ref_flags, float* rows, bool want_hist,
                hipStream_t s) {
    unsigned char* in = st.d_in.get();
    unsigned char* work = st.d_work.get();
    unsigned* counts = (unsigned*)work;
    double* sat = (double*)(work + lay.o_sat);
    if (lay.m > 0) {
        HIPCHK(c, hipMemsetAsync(counts, 0, (size_t)lay.m * 313 * sizeof(unsigned), s));
        if (lay.naa > 0)
            HIPCHK(c, launch_resample(in, in, (const ResampleJob*)(in + lay.o_jobs), lay.naa, lay.aa_tiles, 8, 3, c->H, c->W, s));
        HIPCHK(c, launch_ref_stats((const RefDesc*)in, lay.m, in + lay.o_packed, (const float*)(in + lay.o_centres), c->H, c->W, counts, sat, s));
    }
    HIPCHK(c, launch_glob_rows(counts, sat, (const int*)(in + lay.o_index), lay.n, lay.m, c->H, c->W, hist_flag, (ref_flags & IDC_REF_SATURATION) ? 1 : 0,
                               rows, want_hist ? (float*)(work + lay.o_hist) : nullptr, want_hist ? (float*)(work + lay.o_savg) : nullptr, s));
    return IDC_OK;
}

}  // namespace idc

extern "C" {

int idc_forward(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                float* out_ab) {
    return forward_host(h, n, L_mc, ab, mask, maskcent, out_ab, nullptr);
}

int idc_forward_dist(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                     float* out_ab, float* dist_q) {
    return forward_host(h, n, L_mc, ab, mask, maskcent, out_ab, dist_q, /*keep_dist=*/true);   // NULL dist_q: resident only
}

int idc_forward_device(idc_handle h, int n, const float* d_L_mc, const float* d_ab, const float* d_mask, float maskcent,
                       float* d_out_ab, int sync) {
    int rc = check_forward_args(h, n);
    if (rc) return rc;
    if (!d_L_mc || !d_ab || !d_mask || !d_out_ab) return fail(&h->err, IDC_ERR_INVALID_ARG, "null tensor pointer");
    HIPCHK(h, hipSetDevice(h->device));
    // the result lands in the CALLER's buffer: whatever an earlier forward left in d_out / d_labq is no longer "the last
    // forward's map" (idc_upsample_lab2rgb must not serve it), unless the caller handed the handle's own planes back
    h->out_resident = d_out_ab == h->d_out.get();
    h->labq_resident = false;
    rc = run_graph(h, n, d_L_mc, d_ab, d_mask, maskcent, d_out_ab, (h->flags & IDC_FLAG_DIST_HEAD) ? h->d_dist.get() : nullptr, h->d_glob_in.get());
    if (rc) return rc;
    if (sync) {
        HIPCHK(h, wait_stream(h, n));
        return check_chain_abort(h);           // (every blocking wait that follows run_graph reports a timed-out chain launch itself)
    }
    return IDC_OK;
}

int idc_forward_dist313(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                        float* out_ab, float* pred_ab, float* dist_S) {
    int rc = check_forward_args(h, n);
    if (rc) return rc;
    if (!(h->flags & IDC_FLAG_DIST313)) return fail(&h->err, IDC_ERR_UNSUPPORTED, "handle was created without IDC_FLAG_DIST313");
    if (!pred_ab) return fail(&h->err, IDC_ERR_INVALID_ARG, "null pred_ab");
    const size_t hw = (size_t)h->H * h->W;
    h->want_dist313 = dist_S != nullptr;
    rc = forward_host(h, n, L_mc, ab, mask, maskcent, out_ab ? out_ab : h->h_out.get(), nullptr);
    h->want_dist313 = false;
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(pred_ab, h->d_pred_ab.get(), (size_t)n * hw * 2 * 4, hipMemcpyDeviceToHost));
    if (dist_S) HIPCHK(h, hipMemcpy(dist_S, h->d_dist313.get(), (size_t)n * hw * 313 * 4, hipMemcpyDeviceToHost));
    return IDC_OK;
}

int idc_forward_rgb(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                    float l_cent, float* out_ab, uint8_t* rgb, double* lab_q) {
    int rc = check_forward_args(h, n);
    if (rc) return rc;
    if (!rgb) return fail(&h->err, IDC_ERR_INVALID_ARG, "null rgb");
    rc = ensure_post_buffers(h);
    if (rc) return rc;
    // forward (leaves L_mc in d_L and the ab map in d_out), then the colour step on the same stream: ONE synchronisation for
    // both (the ab map travels to the host under the colour kernel instead of behind a sync of its own)
    rc = forward_host(h, n, L_mc, ab, mask, maskcent, out_ab ? out_ab : h->h_out.get(), nullptr, false, /*finish=*/false);
    if (rc) return rc;
    rc = run_lab_post(h, n, h->d_L.get(), l_cent, h->d_out.get(), rgb, lab_q);          // synchronises the stream
    if (rc == IDC_OK && out_ab && h->out_copy_pending) memcpy(out_ab, h->h_out.get(), (size_t)n * h->H * h->W * 2 * 4);
    h->out_copy_pending = false;
    h->labq_resident = rc == IDC_OK && lab_q != nullptr;
    return rc;
}

// The click as the reference API needs it on the critical path: the colourised image.  The ab map and the refreshed Lab (2.0 MB of
// the 2.2 MB idc_forward_rgb sends back per 256x256 click) stay on the device until idc_fetch_outputs asks for them.
int idc_forward_rgb_lazy(idc_handle h, int n, const float* L_mc, const float* ab, const float* mask, float maskcent, float l_cent, uint8_t* rgb) {
    int rc = check_forward_args(h, n);
    if (rc) return rc;
    if (!rgb) return fail(&h->err, IDC_ERR_INVALID_ARG, "null rgb");
    rc = ensure_post_buffers(h);
    if (rc) return rc;
    rc = forward_host(h, n, L_mc, ab, mask, maskcent, nullptr, nullptr, false, /*finish=*/false, /*copy_out=*/false);
    if (rc) return rc;
    const size_t hw = (size_t)h->H * h->W;
    HIPCHK(h, launch_lab_post(h->d_L.get(), l_cent, h->d_out.get(), h->d_rgb.get(), h->d_labq.get(), n, h->H, h->W, h->stream.get()));
    const bool rgb_direct = is_pinned(rgb);
    HIPCHK(h, copy_h2d_or_d2h(h, h->d_rgb.get(), rgb_direct ? (void*)rgb : (void*)h->h_rgb.get(), (size_t)n * hw * 3, false));
    HIPCHK(h, wait_stream(h, n));
    rc = check_chain_abort(h);
    if (rc) return rc;
    if (!rgb_direct) memcpy(rgb, h->h_rgb.get(), (size_t)n * hw * 3);
    h->out_copy_pending = false;
    h->labq_resident = true;
    return IDC_OK;
}

int idc_fetch_outputs(idc_handle h, int n, float* out_ab, double* lab_q) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (n <= 0 || n > h->max_batch) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->max_batch);
    if (n > h->last_n) return fail(&h->err, IDC_ERR_UNSUPPORTED, "only %d image(s) of the last forward are resident", h->last_n);
    if (out_ab && !h->out_resident) return fail(&h->err, IDC_ERR_UNSUPPORTED, "no forward result is resident");
    if (lab_q && !h->labq_resident) return fail(&h->err, IDC_ERR_UNSUPPORTED, "no refreshed Lab is resident (run idc_forward_rgb_lazy / idc_forward_rgb with lab_q first)");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t hw = (size_t)h->H * h->W;
    const bool ab_direct = out_ab && is_pinned(out_ab), lab_direct = lab_q && is_pinned(lab_q);
    if (out_ab) HIPCHK(h, copy_h2d_or_d2h(h, h->d_out.get(), ab_direct ? out_ab : h->h_out.get(), (size_t)n * hw * 2 * 4, false));
    if (lab_q) {
        int rc = ensure_post_buffers(h);
        if (rc) return rc;
        HIPCHK(h, copy_h2d_or_d2h(h, h->d_labq.get(), lab_direct ? (void*)lab_q : (void*)h->h_labq.get(), (size_t)n * hw * 3 * 8, false));
    }
    HIPCHK(h, wait_stream(h, n));
    if (out_ab && !ab_direct) memcpy(out_ab, h->h_out.get(), (size_t)n * hw * 2 * 4);
    if (lab_q && !lab_direct) memcpy(lab_q, h->h_labq.get(), (size_t)n * hw * 3 * 8);
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- transfer pipeline
// End-to-end batches: two slots, three streams.  Slot k's H2D copies run on the copy-in
// stream while the other slot computes; its D2H runs on the copy-out stream while the next batch computes.  Callers that
// pass pinned host memory (idc_alloc_host, or their own hipHostMalloc / hipHostRegister) are copied from / to directly;
// pageable pointers go through the slot's pinned staging with a host memcpy on the calling thread.
void* idc_alloc_host(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

int idc_free_host(void* p) {
    if (!p) return IDC_OK;
    return hipHostFree(p) == hipSuccess ? IDC_OK : fail(nullptr, IDC_ERR_HIP, "hipHostFree failed");
}

int idc_forward_async(idc_handle h, int slot, int n, const float* L_mc, const float* ab, const float* mask, float maskcent,
                      float* out_ab) {
    int rc = check_forward_args(h, n);
    if (rc) return rc;
    if (slot < 0 || slot > 1) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d not in 0..1", slot);
    if (!L_mc || !ab || !mask || !out_ab) return fail(&h->err, IDC_ERR_INVALID_ARG, "null tensor pointer");
    if (h->audit) return fail(&h->err, IDC_ERR_UNSUPPORTED, "the range audit covers the blocking, resident and device-pointer forwards, not the pipelined slots");
    HIPCHK(h, hipSetDevice(h->device));
    rc = ensure_pipeline(h);
    if (rc) return rc;
    auto& sl = h->pipe[slot];
    if (sl.pending) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d is still in flight: idc_wait it first", slot);
    const size_t hw = (size_t)h->H * h->W, nb = (size_t)h->max_batch;
    const float *sL = L_mc, *sab = ab, *sm = mask;
    if (!(is_pinned(L_mc) && is_pinned(ab) && is_pinned(mask))) {
        HIPCHK(h, sl.h_in.ensure(nb * hw * 4 * 4));
        float* hL = sl.h_in.get(); float* hab = hL + (size_t)n * hw; float* hm = hab + (size_t)n * hw * 2;
        memcpy(hL, L_mc, (size_t)n * hw * 4); memcpy(hab, ab, (size_t)n * hw * 2 * 4); memcpy(hm, mask, (size_t)n * hw * 4);
        sL = hL; sab = hab; sm = hm;
    }
    const bool out_direct = is_pinned(out_ab);
    if (!out_direct) HIPCHK(h, sl.h_out.ensure(nb * hw * 2 * 4));
    // copy-in stream: the slot's previous inputs were consumed (its previous forward finished: idc_wait was called)
    HIPCHK(h, hipEventRecord(sl.ev_in0.get(), h->s_in.get()));
    HIPCHK(h, hipMemcpyAsync(sl.d_L.get(), sL, (size_t)n * hw * 4, hipMemcpyHostToDevice, h->s_in.get()));
    HIPCHK(h, hipMemcpyAsync(sl.d_ab.get(), sab, (size_t)n * hw * 2 * 4, hipMemcpyHostToDevice, h->s_in.get()));
    HIPCHK(h, hipMemcpyAsync(sl.d_mask.get(), sm, (size_t)n * hw * 4, hipMemcpyHostToDevice, h->s_in.get()));
    HIPCHK(h, hipEventRecord(sl.ev_in.get(), h->s_in.get()));
    HIPCHK(h, hipStreamWaitEvent(h->stream.get(), sl.ev_in.get(), 0));
    HIPCHK(h, hipEventRecord(sl.ev_comp0.get(), h->stream.get()));
    rc = run_graph(h, n, sl.d_L.get(), sl.d_ab.get(), sl.d_mask.get(), maskcent, sl.d_out.get(), nullptr, h->d_glob_in.get());
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(sl.ev_comp.get(), h->stream.get()));
    HIPCHK(h, hipStreamWaitEvent(h->s_out.get(), sl.ev_comp.get(), 0));
    HIPCHK(h, hipEventRecord(sl.ev_out0.get(), h->s_out.get()));
    sl.outs.clear();
    HIPCHK(h, copy_out(h, sl, out_ab, out_direct, sl.d_out.get(), sl.h_out.get(), 0, (size_t)n * hw * 2 * 4));
    HIPCHK(h, hipEventRecord(sl.ev_out.get(), h->s_out.get()));
    sl.temporal.on = 0;                      // the caller's planes are no sequence: idc_temporal_info has nothing to report for this call
    sl.pending = true; sl.timed = true;
    return IDC_OK;
}

// The serving form of the product: uint8 images and hint lists in, colourised uint8 images out, on the same two slots.  The slot owns the
// packed source, the clipped hint list, its planes and its results.  A call (BatchCall, idc_batch.h) goes through forward_async_rgb's passes:
// every argument is checked before anything is allocated, written or enqueued, and the slot counts as in flight only once all of it is.
using Slot = idc_context::PipeSlot;
// What a batch needs from the handle-dependent checks: where its references, taps and score sit (all zero without them: nothing of them is
// allocated, launched or copied)
struct BatchLayouts { RefLayout ref; DistGeom geom; TapsLayout taps; ScoreLayout score; size_t score_in_bytes = 0; };

// Pieces <-> a packed device array on `s`, as copy_runs decides; a staged piece is copied in by batch_stage before, copied out by idc_wait after
static hipError_t copy_pieces(const std::vector<Piece>& pieces, bool to_device, unsigned char* dev, unsigned char* staging, hipStream_t s) {
    for (const CopyOp& o : copy_runs(pieces, to_device)) {
        void* host = o.piece < 0 ? (void*)(staging + o.at) : to_device ? (void*)pieces[o.piece].in : (void*)pieces[o.piece].out;
        const hipError_t e = to_device ? hipMemcpyAsync(dev + o.at, host, o.bytes, hipMemcpyHostToDevice, s)
                                       : hipMemcpyAsync(host, dev + o.at, o.bytes, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the checks that read the handle, behind plan_batch's: references, distribution taps and score, the range audit, the slot itself
static int batch_handle_checks(idc_context* h, const BatchCall& c, const BatchPlan& p, BatchLayouts* L) {
    if (c.has_refs) {
        const int rc = check_refs(h, 0, c.n, c.refs.m, c.refs.refs, c.refs.ref_index, c.refs.centres, c.refs.hist_flag, c.refs.flags, &L->ref);
        if (rc) return rc;
        if (!(h->flags & IDC_FLAG_GLOBAL_HINTS)) return fail(&h->err, IDC_ERR_UNSUPPORTED, "handle was created without IDC_FLAG_GLOBAL_HINTS");
    }
    if (p.dist) {
        if (!dist_geom(h, &L->geom))
            return fail(&h->err, IDC_ERR_UNSUPPORTED, "handle has no distribution head (IDC_FLAG_DIST_HEAD, or IDC_FLAG_DIST313 with idc_keep_dist on)");
        if (!p.score || c.taps) {
            const int rc = check_taps(h, L->geom, c.n, 0, 0, c.taps, &L->taps);
            if (rc) return rc;
        }
        if (p.score) {
            const int rc = check_score(h, L->geom, c.n, c.spec, c.centres, c.sout, &L->score);
            if (rc) return rc;
        }
    }
    L->score_in_bytes = align_up((size_t)L->geom.B * 2 * sizeof(float), 16);
    if (h->audit) return fail(&h->err, IDC_ERR_UNSUPPORTED, "the range audit covers the blocking, resident and device-pointer forwards, not the pipelined slots");
    if (h->pipe[c.slot].pending) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d is still in flight: idc_wait it first", c.slot);
    return IDC_OK;
}

// the sequence state of the temporal filter, made on first use: never read before a frame has written it (idc_context::temporal_have)
static int ensure_temporal_state(idc_context* h) {
    const size_t hw = (size_t)h->H * h->W;
    HIPCHK(h, h->d_t_yprev.ensure(2 * hw * sizeof(float)));
    HIPCHK(h, h->d_t_lprev.ensure(hw * sizeof(float)));
    return IDC_OK;
}

// the two launches of the rule on `s`: x [n,2,H,W] becomes y in place, the state advances, D and the flags land in `info` (idc_temporal.h)
// With motion on (idc_set_temporal_motion; idc_motion.hip): the search, the diff on the warped predecessor, one blend launch per frame -- frame f
// reads the filtered x[f - 1] at displaced pixels -- and the state by two copies behind the last of them; the vectors land in `vec`.
// searched: a tracking call has run this very search in front of the network (batch_colourise); `vec` holds its vectors.
static int run_temporal(idc_context* h, const TemporalParams& tp, const MotionParams& mp, int n, const float* L, float* x, unsigned char* scratch,
                        unsigned char* info, unsigned char* vec, bool searched, hipStream_t s) {
    double* g = (double*)scratch;
    double* part = (double*)(scratch + temporal_part_at(n, h->H, h->W));
    const int have = h->temporal_have ? 1 : 0;
    if (mp.on) {
        const int H = h->H, W = h->W, P = temporal_partials(H, W);
        const size_t hw = (size_t)H * W;
        int8_t* v = (int8_t*)vec;
        if (!searched) HIPCHK(h, launch_motion_search(L, h->d_t_lprev.get(), have, n, H, W, mp.search, mp.penalty, v, s));
        HIPCHK(h, launch_motion_diff(L, h->d_t_lprev.get(), v, have, n, H, W, tp.radius, tp.strength, tp.sigma, g, part, s));
        for (int f = 0; f < n; ++f)
            HIPCHK(h, launch_motion_blend(x + (size_t)f * 2 * hw, f ? x + (size_t)(f - 1) * 2 * hw : h->d_t_yprev.get(), g + (size_t)f * hw,
                                          part + (size_t)f * P, v + motion_vector_bytes(f, H, W), f == 0 && !have, H, W, tp.cut, (double*)info + f,
                                          (int*)(info + temporal_info_cut_at(n)) + f, s));
        // the state, behind the last launch: frame 0 of an n = 1 call read y_prev and l_prev at displaced pixels, so no launch wrote them
        HIPCHK(h, hipMemcpyAsync(h->d_t_yprev.get(), x + (size_t)(n - 1) * 2 * hw, 2 * hw * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(h, hipMemcpyAsync(h->d_t_lprev.get(), L + (size_t)(n - 1) * hw, hw * sizeof(float), hipMemcpyDeviceToDevice, s));
        return IDC_OK;
    }
    HIPCHK(h, launch_temporal_diff(L, h->d_t_lprev.get(), have, n, h->H, h->W, tp.radius, tp.strength, tp.sigma, g, part, s));
    HIPCHK(h, launch_temporal_blend(x, g, part, L, h->d_t_yprev.get(), h->d_t_lprev.get(), have, n, h->H, h->W, tp.cut, (double*)info,
                                    (int*)(info + temporal_info_cut_at(n)), s));
    return IDC_OK;
}

// every buffer of the slot this batch uses, at the size it needs: the slot is idle (its last batch was waited for), so they may be replaced by
// larger ones (the reference stage grows in stage_refs)
static int batch_reserve(idc_context* h, const BatchCall& c, const BatchPlan& p, const BatchLayouts& L, Slot& sl) {
    const size_t hw = (size_t)h->H * h->W, nb = (size_t)h->max_batch;
    HIPCHK(h, sl.d_src.ensure(p.src_bytes));       // the packed sources and, behind them, the net-size images of an antialiased call
    HIPCHK(h, sl.d_meta.ensure(p.meta_bytes, p.meta_floor));
    HIPCHK(h, sl.h_meta.ensure(p.meta_bytes, p.meta_floor));
    HIPCHK(h, sl.d_rgb.ensure(nb * hw * 3));
    if (p.source_out) {
        HIPCHK(h, sl.d_labq.ensure(nb * hw * 3 * 8));
        HIPCHK(h, sl.d_full.ensure(p.rgb_bytes));
    }
    if (c.eval) {
        if (!p.source_out) HIPCHK(h, sl.d_truth.ensure(nb * hw * 3));
        HIPCHK(h, sl.d_eval.ensure(p.cols_at + p.cols_bytes, p.cols_at + 4096));
        HIPCHK(h, sl.h_eval.ensure(p.cols_at + p.cols_bytes, p.cols_at + 4096));
    }
    if (p.dist) {     // the taps' queries and centres travel with the batch; their results wait in the slot's block
        HIPCHK(h, sl.d_taps_in.ensure(L.taps.in_bytes, 65536));
        HIPCHK(h, sl.h_taps_in.ensure(L.taps.in_bytes, 65536));
        HIPCHK(h, sl.d_taps.ensure(L.taps.out_bytes, 65536));
        HIPCHK(h, sl.h_taps.ensure(L.taps.out_bytes, 65536));
    }
    if (p.score) {    // ... and so do the score's centres and results
        HIPCHK(h, sl.d_score_in.ensure(L.score_in_bytes, 8192));
        HIPCHK(h, sl.h_score_in.ensure(L.score_in_bytes, 8192));
        HIPCHK(h, sl.d_score.ensure(L.score.out_bytes, 65536));
        HIPCHK(h, sl.h_score.ensure(L.score.out_bytes, 65536));
    }
    bool any_staged_in = false, any_staged_rgb = false;
    for (const Piece& q : p.pieces) { any_staged_in |= !q.in_pinned; any_staged_rgb |= !q.out_pinned; }
    if (any_staged_in) HIPCHK(h, sl.h_src.ensure(p.in_bytes));
    if (any_staged_rgb) HIPCHK(h, sl.h_rgb.ensure(p.ycc_bytes ? p.ycc_bytes : p.rgb_bytes));
    if (p.ycc_bytes) HIPCHK(h, sl.d_ycc.ensure(p.ycc_bytes, 65536));
    if (c.temporal.on) {  // the state, the two kernels' scratch and the info block, at the handle's largest batch
        const int rc = ensure_temporal_state(h);
        if (rc) return rc;
        HIPCHK(h, sl.d_t_scratch.ensure(temporal_scratch_bytes(h->max_batch, h->H, h->W)));
        HIPCHK(h, sl.d_t_info.ensure(temporal_info_bytes(h->max_batch), 4096));
        HIPCHK(h, sl.h_t_info.ensure(temporal_info_bytes(h->max_batch), 4096));
        if (c.motion.on) {
            HIPCHK(h, sl.d_t_vec.ensure(motion_vector_bytes(h->max_batch, h->H, h->W), 4096));
            HIPCHK(h, sl.h_t_vec.ensure(motion_vector_bytes(h->max_batch, h->H, h->W), 4096));
            if (c.track.on) {     // the tracked planes of the slot and the sequence's (A, M, G)
                HIPCHK(h, sl.d_tr.ensure(track_scratch_bytes(h->max_batch, h->H, h->W)));
                HIPCHK(h, h->d_tr_state.ensure(track_state_bytes(h->H, h->W)));
            }
        }
    }
    if (!p.ab_pinned) HIPCHK(h, sl.h_out.ensure(nb * hw * 2 * 4));
    if (c.has_refs) HIPCHK(h, sl.d_glob_in.ensure(nb * kGlobIn * sizeof(float)));
    if (c.has_layers) {   // the packed layers in an array of their own, and the cell counts
        bool any_staged_layer = false;
        for (const Piece& q : p.layer_pieces) any_staged_layer |= !q.in_pinned;
        if (p.n_layers > 0) HIPCHK(h, sl.d_layer.ensure(p.layer_bytes, 65536));
        if (any_staged_layer) HIPCHK(h, sl.h_layer.ensure(p.layer_bytes, 65536));
        HIPCHK(h, sl.d_cells.ensure(nb * sizeof(int32_t)));
        if (c.cells && !p.cells_pinned) HIPCHK(h, sl.h_cells.ensure(nb * sizeof(int32_t)));
    }
    return IDC_OK;
}

// everything the copy-in stream will read from the slot's pinned memory, written here on the calling thread
static int batch_stage(idc_context* h, const BatchCall& c, const BatchPlan& p, const BatchLayouts& L, Slot& sl) {
    if (L.taps.Q > 0) {
        if (!L.taps.at_peaks) memcpy(sl.h_taps_in.get(), c.taps->queries, (size_t)L.taps.Q * sizeof(DistQuery));
        memcpy(sl.h_taps_in.get() + L.taps.i_centres, c.taps->centres, (size_t)L.geom.B * 2 * sizeof(float));
    }
    if (p.score) memcpy(sl.h_score_in.get(), c.centres, (size_t)L.geom.B * 2 * sizeof(float));
    for (const Piece& q : p.pieces)      // every host buffer is judged on its own: only the pageable sources go through the staging
        if (!q.in_pinned) memcpy(sl.h_src.get() + q.in_at, q.in, q.in_bytes);
    for (const Piece& q : p.layer_pieces)
        if (!q.in_pinned) memcpy(sl.h_layer.get() + q.in_at, q.in, q.in_bytes);
    fill_batch_meta(c, p, h->H, h->W, sl.h_meta.get());
    return c.has_refs ? stage_refs(h, sl.ref, L.ref, c.refs.refs, c.refs.ref_index, c.refs.centres, false) : IDC_OK;
}

static int batch_copy_in(idc_context* h, const BatchCall& c, const BatchPlan& p, const BatchLayouts& L, Slot& sl) {
    hipStream_t s = h->s_in.get();
    HIPCHK(h, hipEventRecord(sl.ev_in0.get(), s));
    HIPCHK(h, copy_pieces(p.pieces, true, sl.d_src.get(), sl.h_src.get(), s));
    if (p.n_layers > 0) HIPCHK(h, copy_pieces(p.layer_pieces, true, sl.d_layer.get(), sl.h_layer.get(), s));
    HIPCHK(h, hipMemcpyAsync(sl.d_meta.get(), sl.h_meta.get(), p.meta_bytes, hipMemcpyHostToDevice, s));
    if (L.taps.Q > 0) HIPCHK(h, hipMemcpyAsync(sl.d_taps_in.get(), sl.h_taps_in.get(), L.taps.in_bytes, hipMemcpyHostToDevice, s));
    if (p.score) HIPCHK(h, hipMemcpyAsync(sl.d_score_in.get(), sl.h_score_in.get(), L.score_in_bytes, hipMemcpyHostToDevice, s));
    if (c.has_refs) {
        const int rc = upload_refs(h, sl.ref, L.ref, s);
        if (rc) return rc;
    }
    HIPCHK(h, hipEventRecord(sl.ev_in.get(), s));
    return IDC_OK;
}

// the device's view of the slot's metadata block
// (view: the table for the kernels that bring a source to the net size -- the ingestion view of an antialiased ragged call, else tab itself)
struct BatchMeta { const int* offs; HintRect* hints; const ImgDesc* tab; const int* orig; const ImgDesc* view; const ResampleJob* jobs; };
static BatchMeta batch_meta(const BatchPlan& p, Slot& sl) {
    unsigned char* m = sl.d_meta.get();
    const bool has_view = p.naa > 0 && p.jobs_at != p.view_at;
    return {p.kept ? (const int*)m : nullptr, (HintRect*)(m + p.hints_at), (const ImgDesc*)(m + p.table_at), (const int*)(m + p.orig_at),
            (const ImgDesc*)(m + (has_view ? p.view_at : p.table_at)), (const ResampleJob*)(m + p.jobs_at)};
}

// compute stream, first half: [global inputs from the references] [revealed colours] prologue, network, Lab -> RGB, [the source-size image]
static int batch_colourise(idc_context* h, const BatchCall& c, const BatchPlan& p, const BatchLayouts& L, Slot& sl) {
    hipStream_t s = h->stream.get();
    const size_t hw = (size_t)h->H * h->W;
    const int n = c.n;
    const BatchMeta m = batch_meta(p, sl);
    if (c.has_refs) {
        const int rc = launch_refs(h, sl.ref, L.ref, c.refs.hist_flag, c.refs.flags, sl.d_glob_in.get(), false, s);
        if (rc) return rc;
    }
    // antialiased ingestion: the net-size images of the down-scaled sources, behind the packed sources; a same-size call then reads them as its sources
    if (p.naa > 0)
        HIPCHK(h, launch_resample(sl.d_src.get(), sl.d_src.get(), m.jobs, p.naa, p.aa_tiles, c.gray_bits ? c.gray_bits : 8, c.gray_bits ? 1 : 3, h->H, h->W, s));
    sl.ingest_filter = c.ingest_filter;
    int mode = c.mode;
    if (p.reveal) {   // the colours of the list the prologue is about to read; a dropped rectangle's (0, 0) is the memset's
        float* d_cols = p.cols_bytes ? (float*)(sl.d_eval.get() + p.cols_at) : nullptr;
        if (p.cols_bytes) HIPCHK(h, hipMemsetAsync(d_cols, 0, p.cols_bytes, s));
        HIPCHK(h, launch_reveal_hints(sl.d_src.get(), m.view, m.offs, n, 0, 0, h->H, h->W, m.hints, p.kept, m.orig, d_cols, s));
        mode = IDC_HINT_AB;
    }
    // a call with a table (every grey call has one) reads its images through the view; a same-size call is a uniform run, of the net-size images where it was antialiased
    HIPCHK(h, launch_prologue(c.gray_bits, sl.d_src.get() + (c.ragged ? 0 : p.aa_at), c.ragged ? m.view : nullptr, n, p.naa ? h->H : c.src_h,
                              p.naa ? h->W : c.src_w, h->H, h->W, c.l_cent, m.offs, m.hints, mode, c.mask_value, sl.d_L.get(), sl.d_ab.get(), sl.d_mask.get(), s));
    if (c.has_layers) {   // the layers under the rectangles the prologue has just written; a call whose images all came without one reports zeros
        HIPCHK(h, hipMemsetAsync(sl.d_cells.get(), 0, (size_t)n * sizeof(int32_t), s));
        if (p.n_layers > 0)
            HIPCHK(h, launch_hint_layers(sl.d_layer.get(), (const LayerDesc*)(sl.d_meta.get() + p.layers_at), n, p.layer_blocks, h->H, h->W, c.alpha_min,
                                         c.cover, c.mask_value, sl.d_ab.get(), sl.d_mask.get(), (int*)sl.d_cells.get(), s));
    }
    // hint tracking: the search moves in front of the network (it reads L and l_prev alone), the own planes are carried along its vectors into
    // the slot's scratch in one launch, and the network and the taps read the scratch; the state by three copies behind the launch, since
    // frame 0 read it at displaced pixels.  A filtered call without tracking drops the state.
    const bool tracking = c.temporal.on && c.motion.on && c.track.on;
    const float* ab_in = sl.d_ab.get();
    const float* mask_in = sl.d_mask.get();
    sl.tracked = tracking; sl.track = c.track;
    if (tracking) {
        const int H = h->H, W = h->W, have = h->temporal_have ? 1 : 0;
        unsigned char* tr = sl.d_tr.get();
        unsigned char* st = h->d_tr_state.get();
        float* t_ab = (float*)tr;
        float* t_mask = (float*)(tr + track_mask_at(n, H, W));
        int32_t* t_age = (int32_t*)(tr + track_age_at(n, H, W));
        HIPCHK(h, launch_motion_search(sl.d_L.get(), h->d_t_lprev.get(), have, n, H, W, c.motion.search, c.motion.penalty, (int8_t*)sl.d_t_vec.get(), s));
        HIPCHK(h, launch_track_hints(sl.d_ab.get(), sl.d_mask.get(), sl.d_L.get(), h->d_t_lprev.get(), (const int8_t*)sl.d_t_vec.get(), (const float*)st,
                                     (const float*)(st + track_mask_at(1, H, W)), (const int32_t*)(st + track_age_at(1, H, W)), have,
                                     h->track_have ? 1 : 0, n, H, W, c.track.life, c.track.tol, t_ab, t_mask, t_age, s));
        HIPCHK(h, hipMemcpyAsync(st, t_ab + (size_t)(n - 1) * 2 * hw, 2 * hw * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(h, hipMemcpyAsync(st + track_mask_at(1, H, W), t_mask + (size_t)(n - 1) * hw, hw * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(h, hipMemcpyAsync(st + track_age_at(1, H, W), t_age + (size_t)(n - 1) * hw, hw * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        ab_in = t_ab; mask_in = t_mask;
    }
    const int dist_n = h->dist_n;
    // a distribution batch runs model_class into the HANDLE's distribution (the 313 head with idc_keep_dist writes dist_S on every forward anyway)
    const int rc = run_graph(h, n, sl.d_L.get(), ab_in, mask_in, c.maskcent, sl.d_out.get(),
                             (p.dist && !(h->flags & IDC_FLAG_DIST313)) ? h->d_dist.get() : nullptr, c.has_refs ? sl.d_glob_in.get() : h->d_glob_in.get());
    if (rc) return rc;
    if (!p.dist && !((h->flags & IDC_FLAG_DIST313) && h->keep_dist313)) h->dist_n = dist_n;      // no distribution was written: the blocking forward's stays resident
    // the temporal filter: y over x in the slot's ab map, in front of everything that reads it; the heads above saw the raw network
    sl.temporal = c.temporal; sl.temporal_n = n; sl.motion = c.motion;
    if (c.temporal.on) {
        const int trc = run_temporal(h, c.temporal, c.motion, n, sl.d_L.get(), sl.d_out.get(), sl.d_t_scratch.get(), sl.d_t_info.get(),
                                     sl.d_t_vec.get(), tracking, s);
        if (trc) return trc;
        h->temporal_have = true;             // the launches are enqueued: the next call's frame 0 follows this call's last one
        h->track_have = tracking;            // ... with its tracked planes, or without any: a filtered call without tracking drops them
    }
    HIPCHK(h, launch_lab_post(sl.d_L.get(), c.l_cent, sl.d_out.get(), sl.d_rgb.get(), p.source_out ? sl.d_labq.get() : nullptr, n, h->H, h->W, s));
    sl.up_interp = h->batch_interp; sl.up_joint = h->joint;       // the handle's setting as it is now: a later idc_set_batch_upsample does not reach this batch
    const ImgDesc* tab = c.ragged ? m.tab : nullptr;
    if (p.source_out && sl.up_interp == IDC_INTERP_JOINT) {         // guide: the slot's own L plane and this call's l_cent
        const double* pa = sl.d_labq.get() + hw;
        HIPCHK(h, launch_joint_fullres(c.gray_bits, sl.d_src.get(), tab, n, c.src_h, c.src_w, p.max_tiles, pa, pa + hw, 1, (long long)(3 * hw), sl.d_L.get(),
                                       c.l_cent, h->H, h->W, IDC_INTERP_JOINT, sl.up_joint, sl.d_full.get(), c.out_bits, nullptr, s));
    } else if (p.source_out)                                        // on the plan's bytes per pixel
        HIPCHK(h, launch_packed_fullres(c.gray_bits, sl.d_src.get(), tab, n, c.src_h, c.src_w, (long long)(p.in_bytes / p.bpp_in), sl.d_labq.get(), h->H,
                                        h->W, IDC_INTERP_LINEAR, sl.d_full.get(), c.out_bits, s));
    return IDC_OK;
}

// compute stream, second half: what an evaluation or distribution batch reads off the result
static int batch_measure(idc_context* h, const BatchCall& c, const BatchPlan& p, const BatchLayouts& L, Slot& sl) {
    hipStream_t s = h->stream.get();
    const size_t hw = (size_t)h->H * h->W;
    const int n = c.n;
    const BatchMeta m = batch_meta(p, sl);
    if (c.eval && c.sse) {     // the score: the source-size result against the source bytes, or the net-size result against the net-size ground truth
        unsigned long long* d_sse = (unsigned long long*)sl.d_eval.get();
        HIPCHK(h, hipMemsetAsync(d_sse, 0, (size_t)n * 3 * sizeof(uint64_t), s));
        if (p.source_out) {
            HIPCHK(h, launch_eval_sse(sl.d_full.get(), sl.d_src.get(), m.tab, n, 0, p.max_pixels, (long long)(p.in_bytes / 3), d_sse, s));
        } else {
            HIPCHK(h, launch_ragged_net_truth(sl.d_src.get(), m.view, n, h->H, h->W, sl.d_truth.get(), s));
            HIPCHK(h, launch_eval_sse(sl.d_rgb.get(), sl.d_truth.get(), nullptr, n, (long long)hw, (long long)hw, (long long)n * hw, d_sse, s));
        }
    }
    if (p.dist && c.taps) {   // entropy, peaks, suggestions: behind this batch's network, so in front of whatever replaces the handle's distribution next
        const float* mask = sl.tracked ? (const float*)(sl.d_tr.get() + track_mask_at(n, h->H, h->W)) : sl.d_mask.get();     // skip_hints sees the tracked mask
        const int rc = launch_taps(h, L.geom, L.taps, c.taps, mask, sl.d_taps_in.get(), sl.d_taps.get(), s);
        if (rc) return rc;
    }
    if (p.score) {    // behind the other taps: the cells' ground truth from the slot's own packed sources, then the score
        HIPCHK(h, launch_dist_truth(sl.d_src.get(), m.view, n, 0, 0, h->H, h->W, L.geom.s, (float*)(sl.d_score.get() + L.score.o_truth), s));
        const int rc = launch_score(h, L.geom, L.score, (const float*)sl.d_score_in.get(), sl.d_score.get(), s);
        if (rc) return rc;
    }
    // the output format's post-pass: behind the epilogue and the score, which read and leave the RGB, and in front of the slot's D2H event
    if (p.ycc_bytes)
        HIPCHK(h, launch_ycc420(p.source_out ? sl.d_full.get() : sl.d_rgb.get(), (const YccDesc*)(sl.d_meta.get() + p.ycc_at), n, p.ycc_blocks,
                                c.out_format, c.out_matrix, sl.d_ycc.get(), s));
    return IDC_OK;
}

// rows of one result block that go to the caller's buffers; a NULL or empty one takes no copy
struct OutRow { void* user; size_t at, bytes; };
static int copy_out_rows(idc_context* h, Slot& sl, const OutRow* rows, size_t count, const unsigned char* dev, unsigned char* twin) {
    for (const OutRow* o = rows; o < rows + count; ++o)
        if (o->user && o->bytes) HIPCHK(h, copy_out(h, sl, o->user, is_pinned(o->user), dev, twin, o->at, o->bytes));
    return IDC_OK;
}

// copy-out stream: score, taps, sse and colours, images, out_ab -- the small results first
static int batch_copy_out(idc_context* h, const BatchCall& c, const BatchPlan& p, const BatchLayouts& L, Slot& sl) {
    const size_t n = (size_t)c.n, hw = (size_t)h->H * h->W, npix = (size_t)L.geom.Hd * L.geom.Wd;
    int rc = IDC_OK;
    HIPCHK(h, hipEventRecord(sl.ev_out0.get(), h->s_out.get()));
    sl.outs.clear();
    if (c.temporal.on)    // D and the cut flags, into the slot's own pinned block: idc_temporal_info reads them there
        HIPCHK(h, hipMemcpyAsync(sl.h_t_info.get(), sl.d_t_info.get(), temporal_info_bytes(c.n), hipMemcpyDeviceToHost, h->s_out.get()));
    if (c.temporal.on && c.motion.on)    // ... and the vectors with them
        HIPCHK(h, hipMemcpyAsync(sl.h_t_vec.get(), sl.d_t_vec.get(), motion_vector_bytes(c.n, h->H, h->W), hipMemcpyDeviceToHost, h->s_out.get()));
    if (p.score) {
        const idc_dist_score_out* so = c.sout;
        const ScoreLayout& sc = L.score;
        const OutRow rows[] = {{so->xent, sc.o_xent, n * sizeof(double)},
                               {sc.ranks.n > 0 ? so->hits : nullptr, sc.o_hits, n * sc.ranks.n * sizeof(unsigned)},
                               {so->truth_ab, sc.o_truth, n * 2 * npix * sizeof(float)},
                               {so->xent_map, sc.o_xmap, n * npix * sizeof(double)},
                               {so->rank_map, sc.o_rmap, n * npix * sizeof(int)},
                               {so->target, sc.o_tgt, n * npix * sizeof(int)}};
        rc = copy_out_rows(h, sl, rows, sizeof(rows) / sizeof(rows[0]), sl.d_score.get(), sl.h_score.get());
        if (rc) return rc;
    }
    if (p.dist && c.taps) {
        const idc_dist_taps* tp = c.taps;
        const TapsLayout& tl = L.taps;
        const OutRow rows[] = {{tp->entropy, tl.o_ent, n * npix * sizeof(float)},
                               {tl.P > 0 ? tp->peaks : nullptr, tl.o_peaks, n * tl.P * 2 * sizeof(int)},
                               {tl.P > 0 ? tp->peak_ent : nullptr, tl.o_pent, n * tl.P * sizeof(float)},
                               {tl.Q > 0 ? tp->sugg_centres : nullptr, tl.o_sc, (size_t)tl.Q * tl.K * 2 * sizeof(double)},
                               {tl.Q > 0 ? tp->sugg_conf : nullptr, tl.o_sf, (size_t)tl.Q * tl.K * sizeof(double)}};
        rc = copy_out_rows(h, sl, rows, sizeof(rows) / sizeof(rows[0]), sl.d_taps.get(), sl.h_taps.get());
        if (rc) return rc;
    }
    if (c.eval) {
        const OutRow rows[] = {{c.sse, 0, n * 3 * sizeof(uint64_t)}, {c.hint_colours, p.cols_at, p.cols_bytes}};
        rc = copy_out_rows(h, sl, rows, sizeof(rows) / sizeof(rows[0]), sl.d_eval.get(), sl.h_eval.get());
        if (rc) return rc;
    }
    if (c.has_layers && c.cells) HIPCHK(h, copy_out(h, sl, c.cells, p.cells_pinned, sl.d_cells.get(), sl.h_cells.get(), 0, n * sizeof(int32_t)));
    if (p.want_rgb) {
        HIPCHK(h, copy_pieces(p.pieces, false, p.ycc_bytes ? sl.d_ycc.get() : p.source_out ? sl.d_full.get() : sl.d_rgb.get(), sl.h_rgb.get(), h->s_out.get()));
        for (const Piece& q : p.pieces)
            if (!q.out_pinned) sl.outs.push_back({q.out, sl.h_rgb.get() + q.out_at, q.out_bytes});
    }
    if (c.out_ab) HIPCHK(h, copy_out(h, sl, c.out_ab, p.ab_pinned, sl.d_out.get(), sl.h_out.get(), 0, n * hw * 2 * 4));
    HIPCHK(h, hipEventRecord(sl.ev_out.get(), h->s_out.get()));
    return IDC_OK;
}

// handle state -> plan_batch -> handle-dependent checks | reserve -> stage -> copy-in -> compute -> copy-out -> commit.  Left of the bar nothing
// is allocated, written or enqueued, and for any argument list the first check that refuses it is the one include/ideepcolor.h's tables name
static int forward_async_rgb(idc_handle h, const BatchCall& call) {
    int rc = check_forward_args(h, call.n);
    if (rc) return rc;
    BatchCall c = call;
    c.ingest_filter = h->ingest_filter;       // the handle's setting as it is now: a later idc_set_ingest_filter does not reach this batch
    c.out_format = h->out_format; c.out_matrix = h->out_matrix;      // ... and so with idc_set_batch_output
    c.temporal = h->temporal;                                        // ... and with idc_set_temporal_filter
    c.motion = h->motion;                                            // ... and idc_set_temporal_motion
    c.track = h->track;                                              // ... and idc_set_hint_tracking
    BatchPlan p;
    std::string why;
    rc = plan_batch(c, h->H, h->W, h->max_batch, &p, &why);
    if (rc) return fail(&h->err, rc, "%s", why.c_str());
    BatchLayouts L;
    rc = batch_handle_checks(h, c, p, &L);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    rc = ensure_pipeline(h);
    if (rc) return rc;
    Slot& sl = h->pipe[c.slot];
    for (Piece& q : p.pieces) { q.in_pinned = is_pinned(q.in); q.out_pinned = !p.want_rgb || is_pinned(q.out); }
    p.ab_pinned = !c.out_ab || is_pinned(c.out_ab);
    for (Piece& q : p.layer_pieces) q.in_pinned = is_pinned(q.in);
    p.cells_pinned = !c.cells || is_pinned(c.cells);
    rc = batch_reserve(h, c, p, L, sl);
    if (!rc) rc = batch_stage(h, c, p, L, sl);
    if (!rc) rc = batch_copy_in(h, c, p, L, sl);
    if (rc) return rc;
    HIPCHK(h, hipStreamWaitEvent(h->stream.get(), sl.ev_in.get(), 0));
    HIPCHK(h, hipEventRecord(sl.ev_comp0.get(), h->stream.get()));
    rc = batch_colourise(h, c, p, L, sl);
    if (!rc) rc = batch_measure(h, c, p, L, sl);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(sl.ev_comp.get(), h->stream.get()));
    HIPCHK(h, hipStreamWaitEvent(h->s_out.get(), sl.ev_comp.get(), 0));
    rc = batch_copy_out(h, c, p, L, sl);
    if (rc) return rc;
    sl.pending = true; sl.timed = true;      // only now: a call that failed on the way leaves the slot idle and usable
    return IDC_OK;
}

// The six entry points: fill a BatchCall, run it.  same_size_call / images_call take what idc_forward_async_rgb / idc_forward_async_images take.
static BatchCall same_size_call(int slot, int n, int src_h, int src_w, const uint8_t* rgb_in, const int32_t* hint_offsets, const idc_hint* hints,
                                int mode, float mask_value, float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs,
                                uint8_t* rgb_out, float* out_ab) {
    BatchCall c;
    c.slot = slot; c.n = n; c.src_h = src_h; c.src_w = src_w; c.rgb_in = rgb_in; c.rgb_out = rgb_out;
    c.hint_offsets = hint_offsets; c.hints = hints; c.mode = mode; c.mask_value = mask_value; c.maskcent = maskcent; c.l_cent = l_cent;
    c.flags = flags; c.out_ab = out_ab;
    set_batch_refs(c, refs);
    return c;
}

static BatchCall images_call(int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets, const idc_hint* hints, int mode,
                             float mask_value, float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs, uint8_t* const* rgb_out,
                             float* out_ab) {
    BatchCall c = same_size_call(slot, n, 0, 0, nullptr, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags, refs, nullptr, out_ab);
    c.ragged = true; c.images = images; c.outs = rgb_out;
    return c;
}

int idc_forward_async_rgb(idc_handle h, int slot, int n, int src_h, int src_w, const uint8_t* rgb_in, const int32_t* hint_offsets,
                          const idc_hint* hints, int mode, float mask_value, float maskcent, float l_cent, unsigned flags,
                          uint8_t* rgb_out, float* out_ab) {
    return forward_async_rgb(h, same_size_call(slot, n, src_h, src_w, rgb_in, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags, nullptr,
                                               rgb_out, out_ab));
}

int idc_forward_async_rgb_ref(idc_handle h, int slot, int n, int src_h, int src_w, const uint8_t* rgb_in, const int32_t* hint_offsets,
                              const idc_hint* hints, int mode, float mask_value, float maskcent, float l_cent, unsigned flags, int m,
                              const idc_ref_image* refs, const int32_t* ref_index, const float* centres, float hist_flag, unsigned ref_flags,
                              uint8_t* rgb_out, float* out_ab) {
    const idc_batch_refs br = {m, refs, ref_index, centres, hist_flag, ref_flags};
    return forward_async_rgb(h, same_size_call(slot, n, src_h, src_w, rgb_in, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags, &br,
                                               rgb_out, out_ab));
}

int idc_forward_async_images(idc_handle h, int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets, const idc_hint* hints,
                             int mode, float mask_value, float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs,
                             uint8_t* const* rgb_out, float* out_ab) {
    return forward_async_rgb(h, images_call(slot, n, images, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags, refs, rgb_out, out_ab));
}

int idc_forward_async_eval(idc_handle h, int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets, const idc_hint* hints,
                           int mode, float mask_value, float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs,
                           uint8_t* const* rgb_out, float* out_ab, uint64_t* sse, float* hint_colours) {
    BatchCall c = images_call(slot, n, images, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags, refs, rgb_out, out_ab);
    c.eval = true; c.sse = sse; c.hint_colours = hint_colours;
    return forward_async_rgb(h, c);
}

int idc_forward_async_dist(idc_handle h, int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets, const idc_hint* hints,
                           int mode, float mask_value, float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs,
                           uint8_t* const* rgb_out, float* out_ab, uint64_t* sse, float* hint_colours, const idc_dist_taps* taps) {
    BatchCall c = images_call(slot, n, images, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags, refs, rgb_out, out_ab);
    c.eval = true; c.sse = sse; c.hint_colours = hint_colours;
    c.taps_call = true; c.taps = taps;
    return forward_async_rgb(h, c);
}

int idc_forward_async_dist_score(idc_handle h, int slot, int n, const idc_ref_image* images, const int32_t* hint_offsets, const idc_hint* hints,
                                 int mode, float mask_value, float maskcent, float l_cent, unsigned flags, const idc_batch_refs* refs,
                                 uint8_t* const* rgb_out, float* out_ab, uint64_t* sse, float* hint_colours, const idc_dist_taps* taps,
                                 const idc_dist_score_spec* spec, const float* centres, const idc_dist_score_out* out) {
    BatchCall c = images_call(slot, n, images, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags, refs, rgb_out, out_ab);
    c.eval = true; c.sse = sse; c.hint_colours = hint_colours;
    c.taps_call = true; c.taps = taps;
    c.score_call = true; c.spec = spec; c.centres = centres; c.sout = out;
    return forward_async_rgb(h, c);
}

int idc_forward_async_gray(idc_handle h, int slot, int n, int bits, const idc_gray_image* images, const int32_t* hint_offsets,
                           const idc_hint* hints, int mode, float mask_value, float maskcent, float l_cent, unsigned flags,
                           const idc_batch_refs* refs, void* const* rgb_out, float* out_ab, const idc_dist_taps* taps) {
    BatchCall c = images_call(slot, n, nullptr, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags, refs, (uint8_t* const*)rgb_out, out_ab);
    c.grays = images;
    c.gray_bits = bits ? bits : -1;      // (0 is the RGB calls' own value: like every width but 8 and 16 it is refused by the plan)
    c.out_bits = (flags & IDC_BATCH_OUT_RGB16) ? 16 : 8;
    if (taps) { c.eval = true; c.taps_call = true; c.taps = taps; }        // idc_forward_async_dist without a score and without revealed colours
    return forward_async_rgb(h, c);
}

int idc_forward_async_layers(idc_handle h, int slot, int n, int bits, const void* images, const idc_batch_layers* layers, const int32_t* hint_offsets,
                             const idc_hint* hints, int mode, float mask_value, float maskcent, float l_cent, unsigned flags,
                             const idc_batch_refs* refs, void* const* rgb_out, float* out_ab) {
    BatchCall c = images_call(slot, n, bits == 0 ? (const idc_ref_image*)images : nullptr, hint_offsets, hints, mode, mask_value, maskcent, l_cent, flags,
                              refs, (uint8_t* const*)rgb_out, out_ab);
    if (bits != 0) {      // idc_forward_async_gray's call (a width that is neither 8 nor 16 is refused by the plan)
        c.grays = (const idc_gray_image*)images;
        c.gray_bits = bits;
        c.out_bits = (flags & IDC_BATCH_OUT_RGB16) ? 16 : 8;
    }
    set_batch_layers(c, layers);
    return forward_async_rgb(h, c);
}

int idc_wait(idc_handle h, int slot) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (slot < 0 || slot > 1) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d not in 0..1", slot);
    if (!h->pipe_ready) return IDC_OK;
    HIPCHK(h, hipSetDevice(h->device));
    return wait_slot(h, slot);
}

int idc_pipeline_times(idc_handle h, int slot, float* ms6) {
    if (!h || !ms6) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "null argument");
    if (slot < 0 || slot > 1) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d not in 0..1", slot);
    if (!h->pipe_ready || !h->pipe[slot].timed) return fail(&h->err, IDC_ERR_UNSUPPORTED, "slot %d has not run a batch yet", slot);
    auto& sl = h->pipe[slot];
    if (sl.pending) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d is still in flight: idc_wait it first", slot);
    HIPCHK(h, hipSetDevice(h->device));
    hipEvent_t evs[6] = {sl.ev_in0.get(), sl.ev_in.get(), sl.ev_comp0.get(), sl.ev_comp.get(), sl.ev_out0.get(), sl.ev_out.get()};
    for (int i = 0; i < 6; ++i) HIPCHK(h, hipEventElapsedTime(&ms6[i], h->ev_pipe_base.get(), evs[i]));
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- temporal ab filter
int idc_set_temporal_filter(idc_handle h, int on, double strength, double sigma, int radius, double cut) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!temporal_params_ok(on, strength, sigma, radius, cut))
        return fail(&h->err, IDC_ERR_INVALID_ARG, "temporal filter: on %d in {0,1}, strength %g in [0, 0.95], sigma %g in [0.5, 100], radius %d in 0..%d, "
                    "cut %g 0 or in (0, 100]", on, strength, sigma, radius, kTemporalMaxRadius, cut);
    h->temporal = {on, strength, sigma, cut, radius};
    return IDC_OK;
}

int idc_set_temporal_motion(idc_handle h, int on, int search, double penalty) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!motion_params_ok(on, search, penalty))
        return fail(&h->err, IDC_ERR_INVALID_ARG, "temporal motion: on %d in {0,1}, search %d in 0..%d, penalty %g in [0, 1e6]", on, search,
                    kMotionMaxSearch, penalty);
    h->motion = {on, search, penalty};
    return IDC_OK;
}

int idc_temporal_vectors(idc_handle h, int slot, int8_t* v) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (slot < -1 || slot > 1) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d not in -1..1", slot);
    if (!v) return fail(&h->err, IDC_ERR_INVALID_ARG, "null v");
    if (slot < 0) {                          // the last idc_temporal_apply: it blocked, so nothing is in flight
        if (h->t_apply_n <= 0) return fail(&h->err, IDC_ERR_INVALID_ARG, "no idc_temporal_apply has run on this handle yet");
        if (!h->t_apply_motion) return fail(&h->err, IDC_ERR_INVALID_ARG, "the last idc_temporal_apply ran without motion compensation");
        memcpy(v, h->t_apply_vec.data(), motion_vector_bytes(h->t_apply_n, h->H, h->W));
        return IDC_OK;
    }
    auto& sl = h->pipe[slot];
    if (sl.pending) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d is still in flight: idc_wait it first", slot);
    if (!h->pipe_ready || !sl.timed || !sl.temporal.on || sl.temporal_n <= 0)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d: its last call ran without the temporal filter", slot);
    if (!sl.motion.on) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d: its last call ran without motion compensation", slot);
    memcpy(v, sl.h_t_vec.get(), motion_vector_bytes(sl.temporal_n, h->H, h->W));
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- hints that follow the motion vectors
int idc_set_hint_tracking(idc_handle h, int on, int life, double tol) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!track_params_ok(on, life, tol))
        return fail(&h->err, IDC_ERR_INVALID_ARG, "hint tracking: on %d in {0,1}, life %d in 0..%d, tol %g in [0, 100]", on, life, kTrackMaxLife, tol);
    h->track = {on, life, tol};
    return IDC_OK;
}

int idc_tracked_hints(idc_handle h, int slot, float* ab, float* mask, int32_t* age) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (slot < 0 || slot > 1) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d not in 0..1", slot);
    if (!ab && !mask && !age) return fail(&h->err, IDC_ERR_INVALID_ARG, "null ab, mask and age");
    auto& sl = h->pipe[slot];
    if (sl.pending) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d is still in flight: idc_wait it first", slot);
    if (!h->pipe_ready || !sl.timed || !sl.temporal.on || sl.temporal_n <= 0)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d: its last call ran without the temporal filter", slot);
    if (!sl.tracked) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d: its last call ran without hint tracking", slot);
    // on request only: the planes wait in the slot's scratch, which nothing writes before the slot's next call
    HIPCHK(h, hipSetDevice(h->device));
    const int n = sl.temporal_n;
    const size_t hw = (size_t)h->H * h->W;
    const unsigned char* tr = sl.d_tr.get();
    if (ab) HIPCHK(h, hipMemcpy(ab, tr, (size_t)n * 2 * hw * sizeof(float), hipMemcpyDeviceToHost));
    if (mask) HIPCHK(h, hipMemcpy(mask, tr + track_mask_at(n, h->H, h->W), (size_t)n * hw * sizeof(float), hipMemcpyDeviceToHost));
    if (age) HIPCHK(h, hipMemcpy(age, tr + track_age_at(n, h->H, h->W), (size_t)n * hw * sizeof(int32_t), hipMemcpyDeviceToHost));
    return IDC_OK;
}

int idc_track_hints_apply(idc_handle h, int n, const float* l, const float* ab, const float* mask, float* ab_out, float* mask_out,
                          int32_t* age_out, int8_t* v_out) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (n <= 0 || n > h->max_batch) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->max_batch);
    if (!l || !ab || !mask || !ab_out || !mask_out || !age_out) return fail(&h->err, IDC_ERR_INVALID_ARG, "null l, ab, mask, ab_out, mask_out or age_out");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain_pipeline(h);
    if (rc) return rc;
    hipStream_t s = h->stream.get();
    HIPCHK(h, hipStreamSynchronize(s));
    const int H = h->H, W = h->W;
    const size_t hw = (size_t)H * W, vec_bytes = motion_vector_bytes(n, H, W);
    const MotionParams mp = h->motion;
    const TrackParams tk = h->track;
    // in: l [n,H,W], ab [n,2,H,W], mask [n,H,W], then the vectors; out: idc_track.h's layout.  A self-contained sequence: frame 0 has no
    // predecessor, so l_prev and the state are never read -- the launchers still want pointers, and get the call's own planes
    const size_t in_ab_at = (size_t)n * hw * 4, in_mask_at = in_ab_at + (size_t)n * 2 * hw * 4, in_vec_at = in_mask_at + (size_t)n * hw * 4;
    HIPCHK(h, h->d_tr_in.ensure(in_vec_at + vec_bytes));
    HIPCHK(h, h->d_tr_out.ensure(track_scratch_bytes(n, H, W)));
    unsigned char* in = h->d_tr_in.get();
    unsigned char* out = h->d_tr_out.get();
    const float* d_l = (const float*)in;
    const float* d_ab = (const float*)(in + in_ab_at);
    const float* d_mask = (const float*)(in + in_mask_at);
    int8_t* d_v = (int8_t*)(in + in_vec_at);
    HIPCHK(h, hipMemcpyAsync(in, l, (size_t)n * hw * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(in + in_ab_at, ab, (size_t)n * 2 * hw * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(in + in_mask_at, mask, (size_t)n * hw * 4, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));      // a pageable source is the caller's again
    HIPCHK(h, launch_motion_search(d_l, d_l, 0, n, H, W, mp.search, mp.penalty, d_v, s));
    HIPCHK(h, launch_track_hints(d_ab, d_mask, d_l, d_l, d_v, d_ab, d_mask, (const int32_t*)d_mask, 0, 0, n, H, W, tk.life, tk.tol, (float*)out,
                                 (float*)(out + track_mask_at(n, H, W)), (int32_t*)(out + track_age_at(n, H, W)), s));
    HIPCHK(h, hipMemcpyAsync(ab_out, out, (size_t)n * 2 * hw * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(mask_out, out + track_mask_at(n, H, W), (size_t)n * hw * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(age_out, out + track_age_at(n, H, W), (size_t)n * hw * 4, hipMemcpyDeviceToHost, s));
    if (v_out) HIPCHK(h, hipMemcpyAsync(v_out, d_v, vec_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return IDC_OK;
}

int idc_temporal_reset(idc_handle h) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    h->temporal_have = false;                // every launch already enqueued carried its own copy of the flag
    h->track_have = false;
    return IDC_OK;
}

int idc_temporal_info(idc_handle h, int slot, int32_t* cut, double* D) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (slot < 0 || slot > 1) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d not in 0..1", slot);
    if (!cut && !D) return fail(&h->err, IDC_ERR_INVALID_ARG, "null cut and D");
    auto& sl = h->pipe[slot];
    if (sl.pending) return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d is still in flight: idc_wait it first", slot);
    if (!h->pipe_ready || !sl.timed || !sl.temporal.on || sl.temporal_n <= 0)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "slot %d: its last call ran without the temporal filter", slot);
    const int n = sl.temporal_n;
    if (D) memcpy(D, sl.h_t_info.get(), (size_t)n * sizeof(double));
    if (cut) memcpy(cut, sl.h_t_info.get() + temporal_info_cut_at(n), (size_t)n * sizeof(int32_t));
    return IDC_OK;
}

int idc_temporal_apply(idc_handle h, int n, const float* ab, const float* l, float* y, int32_t* cut, double* D) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (n <= 0 || n > h->max_batch) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->max_batch);
    if (!ab || !l || !y) return fail(&h->err, IDC_ERR_INVALID_ARG, "null ab, l or y");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain_pipeline(h);
    if (rc) return rc;
    hipStream_t s = h->stream.get();
    HIPCHK(h, hipStreamSynchronize(s));      // the buffers of the previous call may still be in flight
    rc = ensure_temporal_state(h);
    if (rc) return rc;
    const size_t hw = (size_t)h->H * h->W;
    HIPCHK(h, h->d_t_x.ensure((size_t)n * 2 * hw * sizeof(float)));
    HIPCHK(h, h->d_t_l.ensure((size_t)n * hw * sizeof(float)));
    HIPCHK(h, h->d_t_scratch.ensure(temporal_scratch_bytes(n, h->H, h->W)));
    HIPCHK(h, h->d_t_info.ensure(temporal_info_bytes(h->max_batch), 4096));
    const MotionParams mp = h->motion;
    const size_t vec_bytes = motion_vector_bytes(n, h->H, h->W);
    if (mp.on) HIPCHK(h, h->d_t_vec.ensure(motion_vector_bytes(h->max_batch, h->H, h->W), 4096));
    HIPCHK(h, hipMemcpyAsync(h->d_t_x.get(), ab, (size_t)n * 2 * hw * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(h->d_t_l.get(), l, (size_t)n * hw * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));      // a pageable source is the caller's again
    rc = run_temporal(h, h->temporal, mp, n, h->d_t_l.get(), h->d_t_x.get(), h->d_t_scratch.get(), h->d_t_info.get(), h->d_t_vec.get(), false, s);
    if (rc) return rc;
    h->temporal_have = true;
    h->track_have = false;                   // frames without hints went by: the tracked state no longer belongs to the predecessor
    h->t_apply_n = n; h->t_apply_motion = mp.on != 0;
    std::vector<unsigned char> info(temporal_info_bytes(n));
    if (mp.on) {
        h->t_apply_vec.resize(vec_bytes);
        HIPCHK(h, hipMemcpyAsync(h->t_apply_vec.data(), h->d_t_vec.get(), vec_bytes, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipMemcpyAsync(y, h->d_t_x.get(), (size_t)n * 2 * hw * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(info.data(), h->d_t_info.get(), info.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (D) memcpy(D, info.data(), (size_t)n * sizeof(double));
    if (cut) memcpy(cut, info.data() + temporal_info_cut_at(n), (size_t)n * sizeof(int32_t));
    return IDC_OK;
}

int idc_temporal_state(idc_handle h, float* y_prev, float* l_prev, int32_t* have) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain_pipeline(h);
    if (rc) return rc;
    hipStream_t s = h->stream.get();
    HIPCHK(h, hipStreamSynchronize(s));
    const size_t hw = (size_t)h->H * h->W;
    if (have) *have = h->temporal_have ? 1 : 0;
    if (!h->temporal_have) {                 // no frame yet: the planes read as zeros
        if (y_prev) memset(y_prev, 0, 2 * hw * sizeof(float));
        if (l_prev) memset(l_prev, 0, hw * sizeof(float));
        return IDC_OK;
    }
    if (y_prev) HIPCHK(h, hipMemcpyAsync(y_prev, h->d_t_yprev.get(), 2 * hw * sizeof(float), hipMemcpyDeviceToHost, s));
    if (l_prev) HIPCHK(h, hipMemcpyAsync(l_prev, h->d_t_lprev.get(), hw * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return IDC_OK;
}

int idc_sync(idc_handle h) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    return check_chain_abort(h);
}

}  // extern "C"
