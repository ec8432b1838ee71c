// idc_api.hip -- the handle and what a caller does with it besides weights and forwards (C ABI, include/ideepcolor.h): create / destroy, the last-error
// string (fail), I/O scales, global hints, the click session, Lab -> RGB, colour suggestions and distributions (one pixel, batches, uncertainty peaks: the
// checks and launches the pipelined idc_forward_async_dist shares are here too), the global histogram, reference-image global hints (blocking forms), stream
// ordering, the display upsample, image ingestion (uint8 RGB in, full-resolution RGB out) and the colour picker (gamut map, colour snapping).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "idc_engine.h"

namespace idc {

static thread_local std::string g_last_error;

int fail(std::string* err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (err) *err = buf;
    return code;
}

// diagnostic (IDC_KW_STAMPS=1): where a layer of the last chain launch spent its cycles (mean over workgroups)
static void print_kw_stamps(const idc_context* c) {
    if (!c->d_kw_stamps.get() || c->kw_stamp_blocks <= 0) return;
    std::vector<long long> st((size_t)c->kw_stamp_blocks * kKwChainMax * 8);
    if (hipMemcpy(st.data(), c->d_kw_stamps.get(), st.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    static const char* names[] = {"prefetch+barrier wait", "halo issue", "halo landed", "taps", "reduce+epilogue", "stores acked+wg barrier"};
    static const int seq[] = {0, 1, 6, 2, 3, 4, 5};
    for (int li = 0; li < c->kw_stamp_layers; ++li) {
        double d[6] = {0, 0, 0, 0, 0, 0};
        for (int b = 0; b < c->kw_stamp_blocks; ++b) {
            const long long* p = &st[((size_t)b * kKwChainMax + li) * 8];
            for (int k = 0; k < 6; ++k) {
                if (li + 1 == c->kw_stamp_layers && k == 5) continue;
                d[k] += (double)(p[seq[k + 1]] - p[seq[k]]);
            }
        }
        fprintf(stderr, "kw_chain stamps layer %2d:", li);
        for (int k = 0; k < 6; ++k) fprintf(stderr, " %s %.0f |", names[k], d[k] / c->kw_stamp_blocks);
        fprintf(stderr, "\n");
    }
}

static void destroy_ctx(idc_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream.get()) (void)hipStreamSynchronize(c->stream.get());
    print_kw_stamps(c);
    delete c;
}

int check_device(int device_id, std::string* err) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(err, IDC_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(err, IDC_ERR_NO_DEVICE, "device %d not in 0..%d", device_id, count - 1);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return fail(err, IDC_ERR_HIP, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(err, IDC_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device_id, prop.gcnArchName);
    return IDC_OK;
}

int ensure_post_buffers(idc_context* h) {
    const size_t hw = (size_t)h->H * h->W, nb = (size_t)h->max_batch;
    HIPCHK(h, h->d_rgb.ensure(nb * hw * 3));
    HIPCHK(h, h->d_labq.ensure(nb * hw * 3 * 8));
    HIPCHK(h, h->d_post_in.ensure(nb * hw * 3 * 4));
    HIPCHK(h, h->h_rgb.ensure(nb * hw * 3));
    HIPCHK(h, h->h_labq.ensure(nb * hw * 3 * 8));
    return IDC_OK;
}

// post step on device-resident planes: d_Lp [n,1,H,W] (+ l_add), d_abp [n,2,H,W] -> host rgb / lab_q
int run_lab_post(idc_context* h, int n, const float* d_Lp, float l_add, const float* d_abp, uint8_t* rgb, double* lab_q) {
    const size_t hw = (size_t)h->H * h->W;
    int rc = ensure_post_buffers(h);
    if (rc) return rc;
    HIPCHK(h, launch_lab_post(d_Lp, l_add, d_abp, h->d_rgb.get(), lab_q ? h->d_labq.get() : nullptr, n, h->H, h->W, h->stream.get()));
    const bool rgb_direct = is_pinned(rgb), lab_direct = lab_q && is_pinned(lab_q);      // pinned caller buffers: no staging copy
    HIPCHK(h, copy_h2d_or_d2h(h, h->d_rgb.get(), rgb_direct ? (void*)rgb : (void*)h->h_rgb.get(), (size_t)n * hw * 3, false));
    if (lab_q) HIPCHK(h, copy_h2d_or_d2h(h, h->d_labq.get(), lab_direct ? (void*)lab_q : (void*)h->h_labq.get(), (size_t)n * hw * 3 * 8, false));
    HIPCHK(h, wait_stream(h, n));
    rc = check_chain_abort(h);
    if (rc) return rc;
    if (!rgb_direct) memcpy(rgb, h->h_rgb.get(), (size_t)n * hw * 3);
    if (lab_q && !lab_direct) memcpy(lab_q, h->h_labq.get(), (size_t)n * hw * 3 * 8);
    return IDC_OK;
}

void drop_source(idc_context* h, int slot) {
    if (slot < 0 || slot >= (int)h->src.size()) return;
    auto& sl = h->src[slot];
    sl.d_rgb.reset();                                    // (freeing waits for the device: nothing that reads it is in flight after that)
    sl.d_net.reset();
    sl.h = sl.w = 0; sl.gray_bits = 0;
}

// ---------------------------------------------------------------------------------------------- distribution taps
static size_t taps_align(size_t x) { return (x + 15) & ~(size_t)15; }

bool dist_geom(const idc_context* c, DistGeom* g) {
    if (c->flags & IDC_FLAG_DIST313) {
        if (!c->keep_dist313) return false;
        g->B = 313; g->Hd = c->H; g->Wd = c->W; g->s = 1; g->dist = c->d_dist313.get();
        return true;
    }
    if (!(c->flags & IDC_FLAG_DIST_HEAD)) return false;
    g->B = 529; g->Hd = c->H / 4; g->Wd = c->W / 4; g->s = 4; g->dist = c->d_dist.get();
    return true;
}

int check_taps(idc_context* c, const DistGeom& g, int n, int p_min, int q_min, const idc_dist_taps* taps, TapsLayout* lay) {
    if (!taps) return fail(&c->err, IDC_ERR_INVALID_ARG, "null taps");
    const int P = taps->n_peaks;
    if (P < p_min || P > IDC_PEAKS_MAX) return fail(&c->err, IDC_ERR_INVALID_ARG, "%d peaks outside %d..%d", P, p_min, IDC_PEAKS_MAX);
    if (taps->flags & ~(unsigned)(IDC_PEAKS_SKIP_HINTS | IDC_TAPS_SUGGEST_AT_PEAKS)) return fail(&c->err, IDC_ERR_INVALID_ARG, "unknown taps flag bits 0x%x", taps->flags);
    if (P > 0) {
        const int rmax = g.Hd > g.Wd ? g.Hd : g.Wd;
        if (taps->radius < 1 || taps->radius > rmax) return fail(&c->err, IDC_ERR_INVALID_ARG, "radius %d outside 1..%d", taps->radius, rmax);
        if (!taps->peaks) return fail(&c->err, IDC_ERR_INVALID_ARG, "null peaks");
    }
    const bool at_peaks = (taps->flags & IDC_TAPS_SUGGEST_AT_PEAKS) != 0;
    if (at_peaks && (P == 0 || taps->queries)) return fail(&c->err, IDC_ERR_INVALID_ARG, "IDC_TAPS_SUGGEST_AT_PEAKS needs peaks and a NULL query list");
    const long long Q = at_peaks ? (long long)n * P : (long long)taps->n_queries;
    if ((!at_peaks && taps->n_queries < q_min) || Q < 0 || Q > IDC_SUGGEST_MAX_QUERIES)
        return fail(&c->err, IDC_ERR_INVALID_ARG, "%lld queries outside %d..%d", Q, q_min, IDC_SUGGEST_MAX_QUERIES);
    if (Q > 0) {
        if (taps->K < 1 || taps->K > kSuggestMaxK) return fail(&c->err, IDC_ERR_INVALID_ARG, "K %d outside 1..%d", taps->K, kSuggestMaxK);
        if (taps->N < 1) return fail(&c->err, IDC_ERR_INVALID_ARG, "N must be positive");
        if (!taps->centres || !taps->sugg_centres || !taps->sugg_conf) return fail(&c->err, IDC_ERR_INVALID_ARG, "null pointer");
        if (!at_peaks && !taps->queries) return fail(&c->err, IDC_ERR_INVALID_ARG, "null queries");
        for (int q = 0; !at_peaks && q < (int)Q; ++q) {
            const idc_dist_query& u = taps->queries[q];
            if (u.img < 0 || u.img >= n) return fail(&c->err, IDC_ERR_BATCH, "query %d: image %d outside 0..%d", q, u.img, n - 1);
            if (u.y == -1 && u.x == -1) continue;
            if (u.y < 0 || u.y >= c->H || u.x < 0 || u.x >= c->W) return fail(&c->err, IDC_ERR_INVALID_ARG, "query %d: pixel (%d,%d) outside the image", q, u.y, u.x);
        }
    }
    const size_t npix = (size_t)g.Hd * g.Wd;
    lay->n = n; lay->P = P; lay->Q = (int)Q; lay->K = Q > 0 ? taps->K : 0; lay->at_peaks = at_peaks; lay->want_ent = taps->entropy != nullptr;
    lay->i_centres = taps_align(at_peaks ? 0 : (size_t)Q * sizeof(DistQuery));
    lay->in_bytes = lay->i_centres + (Q > 0 ? taps_align((size_t)g.B * 2 * sizeof(float)) : 0);
    lay->o_ent = 0;
    lay->o_work = taps_align((P > 0 || lay->want_ent) ? (size_t)n * npix * sizeof(float) : 0);
    lay->o_peaks = lay->o_work + taps_align(P > 0 ? (size_t)n * npix * sizeof(float) : 0);
    lay->o_pent = lay->o_peaks + taps_align((size_t)n * P * 2 * sizeof(int));
    lay->o_sc = lay->o_pent + taps_align((size_t)n * P * sizeof(float));
    lay->o_sf = lay->o_sc + taps_align((size_t)lay->Q * lay->K * 2 * sizeof(double));
    lay->out_bytes = lay->o_sf + taps_align((size_t)lay->Q * lay->K * sizeof(double));
    return IDC_OK;
}

int launch_taps(idc_context* c, const DistGeom& g, const TapsLayout& lay, const idc_dist_taps* taps, const float* mask, const unsigned char* in,
                unsigned char* out, hipStream_t s) {
    float* ent = (float*)(out + lay.o_ent);
    int* peaks = (int*)(out + lay.o_peaks);
    if (lay.P > 0 || lay.want_ent) HIPCHK(c, launch_dist_entropy(g.dist, lay.n, g.B, g.Hd * g.Wd, ent, s));
    if (lay.P > 0)
        HIPCHK(c, launch_dist_peaks(ent, (taps->flags & IDC_PEAKS_SKIP_HINTS) ? mask : nullptr, lay.n, g.Hd, g.Wd, g.s, lay.P, taps->radius,
                                    (float*)(out + lay.o_work), peaks, (float*)(out + lay.o_pent), s));
    if (lay.Q > 0)
        HIPCHK(c, launch_suggest_batch(g.dist, lay.n, g.B, g.Hd, g.Wd, g.s, lay.at_peaks ? nullptr : (const DistQuery*)in, lay.at_peaks ? peaks : nullptr,
                                       lay.P, taps->seed, lay.Q, (const float*)(in + lay.i_centres), lay.K, taps->N, (double*)(out + lay.o_sc),
                                       (double*)(out + lay.o_sf), s));
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- distribution scores
int check_score(idc_context* c, const DistGeom& g, int n, const idc_dist_score_spec* spec, const float* centres, const idc_dist_score_out* out,
                ScoreLayout* lay) {
    if (!spec || !out || !out->xent || !centres) return fail(&c->err, IDC_ERR_INVALID_ARG, "null score pointer (spec, out, out->xent, centres)");
    const int nn_max = g.B < IDC_SCORE_MAX_NN ? g.B : IDC_SCORE_MAX_NN;
    if (spec->nn < 1 || spec->nn > nn_max) return fail(&c->err, IDC_ERR_INVALID_ARG, "nn %d outside 1..%d", spec->nn, nn_max);
    if (!std::isfinite(spec->sigma) || !(spec->sigma > 0.f)) return fail(&c->err, IDC_ERR_INVALID_ARG, "sigma must be positive and finite");
    if (spec->n_ranks < 0 || spec->n_ranks > IDC_SCORE_MAX_RANKS)
        return fail(&c->err, IDC_ERR_INVALID_ARG, "%d rank thresholds outside 0..%d", spec->n_ranks, IDC_SCORE_MAX_RANKS);
    for (int j = 0; j < spec->n_ranks; ++j)
        if (spec->ranks[j] < 1 || spec->ranks[j] > g.B) return fail(&c->err, IDC_ERR_INVALID_ARG, "rank threshold %d: %d outside 1..%d", j, spec->ranks[j], g.B);
    if (spec->n_ranks > 0 && !out->hits) return fail(&c->err, IDC_ERR_INVALID_ARG, "null hits with %d rank thresholds", spec->n_ranks);
    const size_t npix = (size_t)g.Hd * g.Wd, nblk = (npix + 63) / 64;
    lay->n = n; lay->nn = spec->nn; lay->sigma = spec->sigma;
    lay->ranks.n = spec->n_ranks;
    for (int j = 0; j < 8; ++j) lay->ranks.thr[j] = j < spec->n_ranks ? spec->ranks[j] : 0;
    lay->want_xmap = out->xent_map != nullptr; lay->want_rmap = out->rank_map != nullptr; lay->want_tgt = out->target != nullptr;
    lay->o_part = 0;
    lay->o_xent = taps_align((size_t)n * nblk * sizeof(double));
    lay->o_hits = lay->o_xent + taps_align((size_t)n * sizeof(double));
    lay->o_truth = lay->o_hits + taps_align((size_t)n * 8 * sizeof(unsigned));
    lay->o_xmap = lay->o_truth + taps_align((size_t)n * 2 * npix * sizeof(float));
    lay->o_rmap = lay->o_xmap + taps_align(lay->want_xmap ? (size_t)n * npix * sizeof(double) : 0);
    lay->o_tgt = lay->o_rmap + taps_align(lay->want_rmap ? (size_t)n * npix * sizeof(int) : 0);
    lay->out_bytes = lay->o_tgt + taps_align(lay->want_tgt ? (size_t)n * npix * sizeof(int) : 0);
    return IDC_OK;
}

int launch_score(idc_context* c, const DistGeom& g, const ScoreLayout& lay, const float* centres, unsigned char* out, hipStream_t s) {
    HIPCHK(c, launch_dist_score(g.dist, (const float*)(out + lay.o_truth), centres, lay.n, g.B, g.Hd * g.Wd, lay.nn, lay.sigma, lay.ranks,
                                (double*)(out + lay.o_part), (double*)(out + lay.o_xent), lay.ranks.n > 0 ? (unsigned*)(out + lay.o_hits) : nullptr,
                                lay.want_xmap ? (double*)(out + lay.o_xmap) : nullptr, lay.want_rmap ? (int*)(out + lay.o_rmap) : nullptr,
                                lay.want_tgt ? (int*)(out + lay.o_tgt) : nullptr, s));
    return IDC_OK;
}

}  // namespace idc

extern "C" {

int idc_version(void) { return IDC_VERSION; }

int idc_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

const char* idc_last_error(idc_handle h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int idc_create(int device_id, int height, int width, int max_batch, int precision, unsigned flags, idc_handle* out) {
    if (!out) return fail(nullptr, IDC_ERR_INVALID_ARG, "null out handle");
    *out = nullptr;
    if (height <= 0 || width <= 0 || height % 8 || width % 8)
        return fail(nullptr, IDC_ERR_INVALID_ARG, "H and W must be positive multiples of 8 (got %dx%d)", height, width);
    if (max_batch <= 0) return fail(nullptr, IDC_ERR_INVALID_ARG, "max_batch must be positive");
    if (precision < IDC_FP32 || precision > IDC_FP16) return fail(nullptr, IDC_ERR_INVALID_ARG, "bad precision %d", precision);
    // an image so large that some layer has no kernel that can address it: IDC_ERR_INVALID_ARG with the reason, before any device is asked for
    int rc = check_geometry(precision, flags, height, width, max_batch, nullptr);
    if (rc) return rc;
    rc = check_device(device_id, nullptr);
    if (rc) return rc;
    if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, IDC_ERR_HIP, "hipSetDevice(%d) failed", device_id);
    idc_context* c = new idc_context();
    c->device = device_id; c->H = height; c->W = width; c->max_batch = max_batch; c->precision = precision; c->flags = flags;
    c->plan = make_blob_plan(precision, flags);
    hipError_t e = c->stream.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = init_kernels();
    if (e != hipSuccess) {
        rc = fail(nullptr, IDC_ERR_HIP, "stream/kernel init failed: %s", hipGetErrorString(e));
        destroy_ctx(c);
        return rc;
    }
    rc = build_graph(c);
    if (rc == IDC_OK) rc = alloc_graph(c);
    if (rc != IDC_OK) { g_last_error = c->err; destroy_ctx(c); return rc; }
    *out = c;
    return IDC_OK;
}

int idc_destroy(idc_handle h) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    destroy_ctx(h);
    return IDC_OK;
}

int idc_set_io_scales(idc_handle h, float l_div, float ab_div, float mask_mul, float out_mul) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (l_div == 0.f || ab_div == 0.f) return fail(&h->err, IDC_ERR_INVALID_ARG, "zero divisor");
    h->l_div = l_div; h->ab_div = ab_div; h->mask_mul = mask_mul; h->out_mul = out_mul;
    return IDC_OK;
}

int idc_set_global_hints(idc_handle h, int n, const float* glob_ab_313_mask, const float* s_avg_mask) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!(h->flags & IDC_FLAG_GLOBAL_HINTS)) return fail(&h->err, IDC_ERR_UNSUPPORTED, "handle was created without IDC_FLAG_GLOBAL_HINTS");
    if (n <= 0 || n > h->max_batch) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->max_batch);
    if (!glob_ab_313_mask) return fail(&h->err, IDC_ERR_INVALID_ARG, "null glob_ab_313_mask");
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<float> host((size_t)h->max_batch * kGlobIn, 0.f);
    for (int i = 0; i < n; ++i) {
        memcpy(&host[(size_t)i * kGlobIn], glob_ab_313_mask + (size_t)i * 314, 314 * 4);
        if (s_avg_mask) memcpy(&host[(size_t)i * kGlobIn + 314], s_avg_mask + (size_t)i * 2, 2 * 4);
    }
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(h->d_glob_in.get(), host.data(), host.size() * 4, hipMemcpyHostToDevice));
    return IDC_OK;
}

int idc_clear_global_hints(idc_handle h) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!(h->flags & IDC_FLAG_GLOBAL_HINTS)) return fail(&h->err, IDC_ERR_UNSUPPORTED, "handle was created without IDC_FLAG_GLOBAL_HINTS");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemset(h->d_glob_in.get(), 0, (size_t)h->max_batch * kGlobIn * 4));
    return IDC_OK;
}

int idc_set_dist_temperature(idc_handle h, float S) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!(S > 0.f)) return fail(&h->err, IDC_ERR_INVALID_ARG, "temperature must be positive");
    h->dist_S = S;
    return IDC_OK;
}

int idc_lab2rgb(idc_handle h, int n, const float* L, const float* ab, uint8_t* rgb, double* lab_q) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (n <= 0 || n > h->max_batch) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->max_batch);
    if (!L || !ab || !rgb) return fail(&h->err, IDC_ERR_INVALID_ARG, "null tensor pointer");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure_post_buffers(h);
    if (rc) return rc;
    const size_t hw = (size_t)h->H * h->W;
    memcpy(h->h_in.get(), L, (size_t)n * hw * 4);
    memcpy(h->h_in.get() + (size_t)n * hw, ab, (size_t)n * hw * 2 * 4);
    HIPCHK(h, hipMemcpyAsync(h->d_post_in.get(), h->h_in.get(), (size_t)n * hw * 3 * 4, hipMemcpyHostToDevice, h->stream.get()));
    rc = run_lab_post(h, n, h->d_post_in.get(), 0.f, h->d_post_in.get() + (size_t)n * hw, rgb, lab_q);
    h->labq_resident = rc == IDC_OK && lab_q != nullptr;        // d_labq = rgb2lab of exactly what was passed in
    if (h->labq_resident && h->last_n < n) h->last_n = n;
    return rc;
}

// ---------------------------------------------------------------------------------------------- click session
static int check_img(idc_context* h, int img) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (img < 0 || img >= h->max_batch) return fail(&h->err, IDC_ERR_BATCH, "image %d outside 0..%d", img, h->max_batch - 1);
    return IDC_OK;
}

int idc_set_image_l(idc_handle h, int img, const float* L_mc) {
    int rc = check_img(h, img);
    if (rc) return rc;
    if (!L_mc) return fail(&h->err, IDC_ERR_INVALID_ARG, "null L_mc");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t hw = (size_t)h->H * h->W;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(h->d_L.get() + (size_t)img * hw, L_mc, hw * 4, hipMemcpyHostToDevice));
    h->l_set[img] = 1;
    drop_source(h, img);
    return IDC_OK;
}

// idc_set_hints, and with a layer idc_set_hints_layer: the rectangles as ever, then the layer under them (launch_hint_layers, n = 1)
static int set_hints(idc_context* h, int img, int n_hints, const idc_hint* hints, int mode, float mask_value, const idc_hint_layer* layer,
                     int alpha_min, int cover, int32_t* cells) {
    int rc = check_img(h, img);
    if (rc) return rc;
    if (n_hints < 0 || (n_hints > 0 && !hints)) return fail(&h->err, IDC_ERR_INVALID_ARG, "bad hint list");
    if (mode != IDC_HINT_AB && mode != IDC_HINT_RGB) return fail(&h->err, IDC_ERR_INVALID_ARG, "hint mode %d", mode);
    if (layer) {
        if (!layer->rgba) return fail(&h->err, IDC_ERR_INVALID_ARG, "null layer pixels");
        if (layer->h < 1 || layer->h > kLayerMaxSide || layer->w < 1 || layer->w > kLayerMaxSide)
            return fail(&h->err, IDC_ERR_INVALID_ARG, "layer size %dx%d outside 1..%d", layer->h, layer->w, kLayerMaxSide);
        if (alpha_min < 1 || alpha_min > 255) return fail(&h->err, IDC_ERR_INVALID_ARG, "alpha_min %d outside 1..255", alpha_min);
        if (cover < 0 || cover > 255) return fail(&h->err, IDC_ERR_INVALID_ARG, "cover %d outside 0..255", cover);
        if ((size_t)layer->h * layer->w * 4 > IDC_BATCH_MAX_SOURCE_BYTES)
            return fail(&h->err, IDC_ERR_INVALID_ARG, "the layer holds %zu bytes, more than %zu", (size_t)layer->h * layer->w * 4, (size_t)IDC_BATCH_MAX_SOURCE_BYTES);
        if (!(std::isfinite(mask_value) && mask_value != 0.f)) return fail(&h->err, IDC_ERR_INVALID_ARG, "a call with a layer needs a finite mask_value != 0");
        if (h->audit) return fail(&h->err, IDC_ERR_UNSUPPORTED, "the range audit does not cover hint layers");
        for (int i = 0; i < n_hints && mode == IDC_HINT_RGB; ++i) {      // everything is decided before anything is enqueued
            HintRect r;
            if (clip_hint(hints[i], h->H, h->W, r) && !(r.c0 >= 0.f && r.c0 <= 255.f && r.c1 >= 0.f && r.c1 <= 255.f && r.c2 >= 0.f && r.c2 <= 255.f))
                return fail(&h->err, IDC_ERR_INVALID_ARG, "hint %d: RGB outside 0..255", i);
        }
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));            // the pinned list of the previous call may still be in flight
    {   // 256 entries to begin with, twice the list once it is longer
        const size_t cap = n_hints < 256 ? 256 : 2 * (size_t)n_hints;
        HIPCHK(h, h->d_hints.ensure((size_t)n_hints * sizeof(HintRect), cap * sizeof(HintRect)));
        HIPCHK(h, h->h_hints.ensure((size_t)n_hints * sizeof(HintRect), cap * sizeof(HintRect)));
    }
    int kept = 0;
    for (int i = 0; i < n_hints; ++i) {                    // cv2.rectangle: corners in either order, inclusive, clipped
        HintRect r;
        if (!clip_hint(hints[i], h->H, h->W, r)) continue;  // entirely outside
        if (mode == IDC_HINT_RGB)
            if (!(r.c0 >= 0.f && r.c0 <= 255.f && r.c1 >= 0.f && r.c1 <= 255.f && r.c2 >= 0.f && r.c2 <= 255.f))
                return fail(&h->err, IDC_ERR_INVALID_ARG, "hint %d: RGB outside 0..255", i);
        h->h_hints.get()[kept++] = r;
    }
    const size_t hw = (size_t)h->H * h->W;
    if (kept) HIPCHK(h, hipMemcpyAsync(h->d_hints.get(), h->h_hints.get(), (size_t)kept * sizeof(HintRect), hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, launch_raster_hints(h->d_hints.get(), kept, mode, mask_value, h->d_ab.get() + (size_t)img * hw * 2, h->d_mask.get() + (size_t)img * hw,
                                  h->H, h->W, h->stream.get()));
    if (layer) {
        const size_t lb = (size_t)layer->h * layer->w * 4;
        HIPCHK(h, h->d_layer.ensure(lb, 65536));
        HIPCHK(h, h->d_layer_meta.ensure(32));
        HIPCHK(h, h->h_layer_meta.ensure(32));
        unsigned char* hm = h->h_layer_meta.get();
        unsigned char* dm = h->d_layer_meta.get();
        memset(hm, 0, 32);
        const LayerDesc d = {0, layer->h, layer->w};
        memcpy(hm, &d, sizeof(d));
        HIPCHK(h, hipMemcpyAsync(dm, hm, 32, hipMemcpyHostToDevice, h->stream.get()));      // the table and a zero count
        HIPCHK(h, hipMemcpyAsync(h->d_layer.get(), layer->rgba, lb, hipMemcpyHostToDevice, h->stream.get()));
        HIPCHK(h, launch_hint_layers(h->d_layer.get(), (const LayerDesc*)dm, 1, layer_blocks(layer->h, layer->w, h->H, h->W), h->H, h->W, alpha_min, cover,
                                     mask_value, h->d_ab.get() + (size_t)img * hw * 2, h->d_mask.get() + (size_t)img * hw, (int*)(dm + 16), h->stream.get()));
        HIPCHK(h, hipMemcpyAsync(hm + 16, dm + 16, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream.get()));
        HIPCHK(h, hipStreamSynchronize(h->stream.get()));               // the caller's pixels are read and the count is here
        if (cells) memcpy(cells, hm + 16, sizeof(int32_t));
    }
    h->hint_mask_value[img] = mask_value;
    return IDC_OK;
}

int idc_set_hints(idc_handle h, int img, int n_hints, const idc_hint* hints, int mode, float mask_value) {
    return set_hints(h, img, n_hints, hints, mode, mask_value, nullptr, 0, 0, nullptr);
}

int idc_set_hints_layer(idc_handle h, int img, int n_hints, const idc_hint* hints, int mode, float mask_value, const idc_hint_layer* layer,
                        int alpha_min, int cover, int32_t* cells) {
    return set_hints(h, img, n_hints, hints, mode, mask_value, layer, alpha_min, cover, cells);
}

// idc_set_hints in IDC_HINT_AB mode with every colour taken from the slot's kept source: the list goes to the device clipped, reveal_hints_kernel
// writes (c0, c1) where it lies, and raster_hints_kernel reads it from there
int idc_reveal_hints(idc_handle h, int img, int n_hints, const idc_hint* rects, float mask_value, float* colours) {
    int rc = check_img(h, img);
    if (rc) return rc;
    if (n_hints < 0 || (n_hints > 0 && !rects)) return fail(&h->err, IDC_ERR_INVALID_ARG, "bad hint list");
    const auto& src = h->src[img];
    if (!src.d_rgb.get()) return fail(&h->err, IDC_ERR_UNSUPPORTED, "image slot %d has no resident source (idc_set_image_rgb with IDC_INGEST_KEEP_SOURCE)", img);
    if (src.gray_bits) return fail(&h->err, IDC_ERR_UNSUPPORTED, "image slot %d holds a greyscale source: it has no colour to reveal", img);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));            // the pinned lists of the previous call may still be in flight
    const size_t cap = n_hints < 256 ? 256 : 2 * (size_t)n_hints;
    HIPCHK(h, h->d_hints.ensure((size_t)n_hints * sizeof(HintRect), cap * sizeof(HintRect)));
    HIPCHK(h, h->h_hints.ensure((size_t)n_hints * sizeof(HintRect), cap * sizeof(HintRect)));
    const size_t cols_at = (size_t)n_hints * sizeof(int), cols_bytes = (size_t)n_hints * 2 * sizeof(float);
    HIPCHK(h, h->d_reveal.ensure(cols_at + cols_bytes, cap * 12));
    HIPCHK(h, h->h_reveal.ensure(cols_at + cols_bytes, cap * 12));
    int* orig = (int*)h->h_reveal.get();
    int kept = 0;
    for (int i = 0; i < n_hints; ++i) {                    // cv2.rectangle, as idc_set_hints reads it
        HintRect r;
        if (!clip_hint(rects[i], h->H, h->W, r)) continue;  // entirely outside
        r.c0 = 0.f; r.c1 = 0.f; r.c2 = 0.f;
        orig[kept] = i;
        h->h_hints.get()[kept++] = r;
    }
    const size_t hw = (size_t)h->H * h->W;
    float* d_cols = (float*)(h->d_reveal.get() + cols_at);
    if (kept) {
        HIPCHK(h, hipMemcpyAsync(h->d_hints.get(), h->h_hints.get(), (size_t)kept * sizeof(HintRect), hipMemcpyHostToDevice, h->stream.get()));
        HIPCHK(h, hipMemcpyAsync(h->d_reveal.get(), orig, (size_t)kept * sizeof(int), hipMemcpyHostToDevice, h->stream.get()));
    }
    if (n_hints) HIPCHK(h, hipMemsetAsync(d_cols, 0, cols_bytes, h->stream.get()));      // a dropped rectangle reports (0, 0)
    // a source that was down-scaled under IDC_FILTER_ANTIALIAS reveals the colours of the net-size image that ingestion made (the identity at H x W)
    const bool aa = src.d_net.get() != nullptr;
    HIPCHK(h, launch_reveal_hints(aa ? src.d_net.get() : src.d_rgb.get(), nullptr, nullptr, 1, aa ? h->H : src.h, aa ? h->W : src.w, h->H, h->W, h->d_hints.get(),
                                  kept, (const int*)h->d_reveal.get(), d_cols, h->stream.get()));
    HIPCHK(h, launch_raster_hints(h->d_hints.get(), kept, IDC_HINT_AB, mask_value, h->d_ab.get() + (size_t)img * hw * 2, h->d_mask.get() + (size_t)img * hw,
                                  h->H, h->W, h->stream.get()));
    h->hint_mask_value[img] = mask_value;
    if (colours && n_hints) {
        HIPCHK(h, hipMemcpyAsync(h->h_reveal.get() + cols_at, d_cols, cols_bytes, hipMemcpyDeviceToHost, h->stream.get()));
        HIPCHK(h, hipStreamSynchronize(h->stream.get()));
        memcpy(colours, h->h_reveal.get() + cols_at, cols_bytes);
    }
    return IDC_OK;
}

int idc_get_hint_planes(idc_handle h, int img, float* ab, float* mask) {
    int rc = check_img(h, img);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t hw = (size_t)h->H * h->W;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    if (ab) HIPCHK(h, hipMemcpy(ab, h->d_ab.get() + (size_t)img * hw * 2, hw * 2 * 4, hipMemcpyDeviceToHost));
    if (mask) HIPCHK(h, hipMemcpy(mask, h->d_mask.get() + (size_t)img * hw, hw * 4, hipMemcpyDeviceToHost));
    return IDC_OK;
}

int idc_forward_resident(idc_handle h, int n, float maskcent, float l_cent, float* out_ab, uint8_t* rgb, double* lab_q) {
    int rc = check_forward_args(h, n);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    for (int i = 0; i < n; ++i)
        if (!h->l_set[i]) return fail(&h->err, IDC_ERR_INVALID_ARG, "I need to have an image! (slot %d has no L plane: idc_set_image_l)", i);
    rc = drain_pipeline(h);
    if (rc) return rc;
    const size_t hw = (size_t)h->H * h->W;
    rc = run_graph(h, n, h->d_L.get(), h->d_ab.get(), h->d_mask.get(), maskcent, h->d_out.get(), (h->flags & IDC_FLAG_DIST_HEAD) ? h->d_dist.get() : nullptr, h->d_glob_in.get());
    if (rc) return rc;
    h->out_resident = true; h->labq_resident = rgb != nullptr && lab_q != nullptr;
    if (out_ab) HIPCHK(h, hipMemcpyAsync(h->h_out.get(), h->d_out.get(), (size_t)n * hw * 2 * 4, hipMemcpyDeviceToHost, h->stream.get()));
    if (rgb) {
        rc = run_lab_post(h, n, h->d_L.get(), l_cent, h->d_out.get(), rgb, lab_q);      // synchronises the stream
        if (rc) return rc;
    } else {
        HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    }
    rc = check_chain_abort(h);
    if (rc) return rc;
    if (out_ab) memcpy(out_ab, h->h_out.get(), (size_t)n * hw * 2 * 4);
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- colour suggestions
int idc_keep_dist(idc_handle h, int on) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!(h->flags & IDC_FLAG_DIST313)) return fail(&h->err, IDC_ERR_UNSUPPORTED, "handle was created without IDC_FLAG_DIST313");
    h->keep_dist313 = on != 0;
    return IDC_OK;
}

// where the resident distribution of image `img` lives: bins, element stride between bins, pointer to bin 0 at (y, x)
static int dist_locate(idc_context* h, int img, int y, int x, int* B, long long* stride, const float** p) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (h->dist_n <= 0) return fail(&h->err, IDC_ERR_UNSUPPORTED, "Need to set prediction first (no resident distribution)");
    if (img < 0 || img >= h->dist_n) return fail(&h->err, IDC_ERR_BATCH, "image %d outside 0..%d", img, h->dist_n - 1);
    if (y < 0 || y >= h->H || x < 0 || x >= h->W) return fail(&h->err, IDC_ERR_INVALID_ARG, "pixel (%d,%d) outside the image", y, x);
    if (h->flags & IDC_FLAG_DIST313) {
        *B = 313; *stride = (long long)h->H * h->W;
        *p = h->d_dist313.get() + (size_t)img * 313 * (*stride) + (size_t)y * h->W + x;
    } else {                                               // 529 bins at H/4 x W/4; out_cl is its nearest x4 upsample (model.py:131)
        const int h4 = h->H / 4, w4 = h->W / 4;
        *B = 529; *stride = (long long)h4 * w4;
        *p = h->d_dist.get() + (size_t)img * 529 * (*stride) + (size_t)(y / 4) * w4 + (x / 4);
    }
    return IDC_OK;
}

int idc_dist_bins(idc_handle h) { return !h ? 0 : (h->flags & IDC_FLAG_DIST313) ? 313 : (h->flags & IDC_FLAG_DIST_HEAD) ? 529 : 0; }

int idc_dist_at(idc_handle h, int img, int y, int x, float* pdf) {
    int B; long long stride; const float* p;
    int rc = dist_locate(h, img, y, x, &B, &stride, &p);
    if (rc) return rc;
    if (!pdf) return fail(&h->err, IDC_ERR_INVALID_ARG, "null pdf");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy2D(pdf, 4, p, (size_t)stride * 4, 4, (size_t)B, hipMemcpyDeviceToHost));
    return IDC_OK;
}

int idc_get_dist(idc_handle h, int n, float* dist) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (h->dist_n <= 0) return fail(&h->err, IDC_ERR_UNSUPPORTED, "Need to set prediction first (no resident distribution)");
    if (n <= 0 || n > h->dist_n) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->dist_n);
    if (!dist) return fail(&h->err, IDC_ERR_INVALID_ARG, "null dist");
    HIPCHK(h, hipSetDevice(h->device));
    const size_t hw = (size_t)h->H * h->W;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    if (h->flags & IDC_FLAG_DIST313) HIPCHK(h, hipMemcpy(dist, h->d_dist313.get(), (size_t)n * 313 * hw * 4, hipMemcpyDeviceToHost));
    else HIPCHK(h, hipMemcpy(dist, h->d_dist.get(), (size_t)n * 529 * (hw / 16) * 4, hipMemcpyDeviceToHost));
    return IDC_OK;
}

// device copy of the caller's bin centres (idc_suggest_colors, idc_dist_decode) and the suggestion results: first use
static int ensure_centres(idc_context* h) {
    HIPCHK(h, h->d_centres.ensure((size_t)kSuggestMaxBins * 2 * 4));
    HIPCHK(h, h->d_sugg.ensure((size_t)kSuggestMaxK * 3 * 8));
    HIPCHK(h, h->d_sugg_counts.ensure((size_t)kSuggestMaxBins * 4));
    return IDC_OK;
}

int idc_suggest_colors(idc_handle h, int img, int y, int x, int K, int N, unsigned seed, const float* centres,
                       double* out_centres, double* out_conf, unsigned* out_counts) {
    int B; long long stride; const float* p;
    int rc = dist_locate(h, img, y, x, &B, &stride, &p);
    if (rc) return rc;
    if (!centres || !out_centres || !out_conf) return fail(&h->err, IDC_ERR_INVALID_ARG, "null pointer");
    if (K < 1 || K > kSuggestMaxK) return fail(&h->err, IDC_ERR_INVALID_ARG, "K %d outside 1..%d", K, kSuggestMaxK);
    if (N < 1) return fail(&h->err, IDC_ERR_INVALID_ARG, "N must be positive");
    HIPCHK(h, hipSetDevice(h->device));
    rc = ensure_centres(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(h->d_centres.get(), centres, (size_t)B * 2 * 4, hipMemcpyHostToDevice));
    HIPCHK(h, launch_suggest(p, stride, B, h->d_centres.get(), K, N, seed, h->d_sugg.get(), h->d_sugg.get() + 2 * kSuggestMaxK, h->d_sugg_counts.get(), h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(out_centres, h->d_sugg.get(), (size_t)K * 2 * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(out_conf, h->d_sugg.get() + 2 * kSuggestMaxK, (size_t)K * 8, hipMemcpyDeviceToHost));
    if (out_counts) HIPCHK(h, hipMemcpy(out_counts, h->d_sugg_counts.get(), (size_t)B * 4, hipMemcpyDeviceToHost));
    return IDC_OK;
}

// the whole resident distribution of images 0..n-1: bins, pixels per bin plane, pointer; allocates the handle's result maps on first use
static int dist_maps_begin(idc_context* h, int n, int* B, int* npix, const float** dist) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (h->dist_n <= 0) return fail(&h->err, IDC_ERR_UNSUPPORTED, "Need to set prediction first (no resident distribution)");
    if (n <= 0 || n > h->dist_n) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->dist_n);
    const bool d313 = (h->flags & IDC_FLAG_DIST313) != 0;
    *B = d313 ? 313 : 529;
    *npix = d313 ? h->H * h->W : (h->H / 4) * (h->W / 4);
    *dist = d313 ? h->d_dist313.get() : h->d_dist.get();
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, h->d_map_ab.ensure((size_t)h->max_batch * 2 * (*npix) * 4));
    HIPCHK(h, h->d_map_s.ensure((size_t)h->max_batch * (*npix) * 4));
    return IDC_OK;
}

int idc_dist_entropy(idc_handle h, int n, float* ent) {
    int B, npix; const float* dist;
    int rc = dist_maps_begin(h, n, &B, &npix, &dist);
    if (rc) return rc;
    if (!ent) return fail(&h->err, IDC_ERR_INVALID_ARG, "null ent");
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, launch_dist_entropy(dist, n, B, npix, h->d_map_s.get(), h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(ent, h->d_map_s.get(), (size_t)n * npix * 4, hipMemcpyDeviceToHost));
    return IDC_OK;
}

int idc_dist_decode(idc_handle h, int n, int mode, float gamma, const float* centres, float* ab, float* conf) {
    int B, npix; const float* dist;
    int rc = dist_maps_begin(h, n, &B, &npix, &dist);
    if (rc) return rc;
    if (!centres || !ab) return fail(&h->err, IDC_ERR_INVALID_ARG, "null pointer");
    if (mode != IDC_DECODE_MODE && mode != IDC_DECODE_MEAN) return fail(&h->err, IDC_ERR_INVALID_ARG, "unknown decode mode %d", mode);
    if (!std::isfinite(gamma) || gamma <= 0.f) return fail(&h->err, IDC_ERR_INVALID_ARG, "gamma must be positive and finite");
    rc = ensure_centres(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(h->d_centres.get(), centres, (size_t)B * 2 * 4, hipMemcpyHostToDevice));
    HIPCHK(h, launch_dist_decode(dist, n, B, npix, mode, gamma, h->d_centres.get(), h->d_map_ab.get(), conf ? h->d_map_s.get() : nullptr, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(ab, h->d_map_ab.get(), (size_t)n * 2 * npix * 4, hipMemcpyDeviceToHost));
    if (conf) HIPCHK(h, hipMemcpy(conf, h->d_map_s.get(), (size_t)n * npix * 4, hipMemcpyDeviceToHost));
    return IDC_OK;
}

// The blocking forms of the distribution taps, on the handle's own blocks: checks, [one upload], the launches of launch_taps, one copy back
static int run_taps_blocking(idc_context* h, int n, int p_min, int q_min, const idc_dist_taps* taps) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    DistGeom g;
    if (!dist_geom(h, &g) || h->dist_n <= 0) return fail(&h->err, IDC_ERR_UNSUPPORTED, "Need to set prediction first (no resident distribution)");
    if (n <= 0 || n > h->dist_n) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->dist_n);
    TapsLayout lay;
    int rc = check_taps(h, g, n, p_min, q_min, taps, &lay);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    rc = drain_pipeline(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    const size_t o_out = taps_align(lay.in_bytes), total = o_out + lay.out_bytes, res0 = lay.o_peaks;       // the entropy and work maps stay on the device
    HIPCHK(h, h->d_taps.ensure(total, 65536));
    HIPCHK(h, h->h_taps.ensure(total, 65536));
    if (lay.Q > 0) {
        memcpy(h->h_taps.get(), taps->queries, (size_t)lay.Q * sizeof(DistQuery));
        memcpy(h->h_taps.get() + lay.i_centres, taps->centres, (size_t)g.B * 2 * sizeof(float));
        HIPCHK(h, hipMemcpyAsync(h->d_taps.get(), h->h_taps.get(), lay.in_bytes, hipMemcpyHostToDevice, h->stream.get()));
    }
    rc = launch_taps(h, g, lay, taps, h->d_mask.get(), h->d_taps.get(), h->d_taps.get() + o_out, h->stream.get());
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->h_taps.get() + o_out + res0, h->d_taps.get() + o_out + res0, lay.out_bytes - res0, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    const unsigned char* res = h->h_taps.get() + o_out;
    if (lay.P > 0) {
        memcpy(taps->peaks, res + lay.o_peaks, (size_t)n * lay.P * 2 * sizeof(int));
        if (taps->peak_ent) memcpy(taps->peak_ent, res + lay.o_pent, (size_t)n * lay.P * sizeof(float));
    }
    if (lay.Q > 0) {
        memcpy(taps->sugg_centres, res + lay.o_sc, (size_t)lay.Q * lay.K * 2 * sizeof(double));
        memcpy(taps->sugg_conf, res + lay.o_sf, (size_t)lay.Q * lay.K * sizeof(double));
    }
    return IDC_OK;
}

int idc_dist_peaks(idc_handle h, int n, int P, int radius, unsigned flags, int32_t* peaks, float* peak_ent) {
    if (flags & ~(unsigned)IDC_PEAKS_SKIP_HINTS) return fail(h ? &h->err : nullptr, IDC_ERR_INVALID_ARG, "unknown flag bits 0x%x", flags);
    idc_dist_taps taps = {};
    taps.n_peaks = P; taps.radius = radius; taps.flags = flags; taps.peaks = peaks; taps.peak_ent = peak_ent;
    return run_taps_blocking(h, n, 1, 0, &taps);
}

int idc_suggest_colors_batch(idc_handle h, int nq, const idc_dist_query* q, int K, int N, const float* centres, double* out_centres,
                             double* out_conf) {
    idc_dist_taps taps = {};
    taps.n_queries = nq; taps.queries = q; taps.K = K; taps.N = N; taps.centres = centres; taps.sugg_centres = out_centres; taps.sugg_conf = out_conf;
    return run_taps_blocking(h, h ? (h->dist_n > 0 ? h->dist_n : 1) : 1, 0, 1, &taps);
}

// The blocking form of the distribution score: checks, the centres up, one truth launch per image (each slot keeps a source of its own size), the
// score launches, and the wanted parts of the result block straight to the caller
int idc_dist_score(idc_handle h, int n, const idc_dist_score_spec* spec, const float* centres, const idc_dist_score_out* out) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    DistGeom g;
    if (!dist_geom(h, &g)) return fail(&h->err, IDC_ERR_UNSUPPORTED, "handle has no distribution head (IDC_FLAG_DIST_HEAD, or IDC_FLAG_DIST313 with idc_keep_dist on)");
    ScoreLayout lay;
    int rc = check_score(h, g, n, spec, centres, out, &lay);
    if (rc) return rc;
    if (h->audit) return fail(&h->err, IDC_ERR_UNSUPPORTED, "the distribution score does not run while the range audit is on");
    if (h->dist_n <= 0) return fail(&h->err, IDC_ERR_UNSUPPORTED, "Need to set prediction first (no resident distribution)");
    if (n <= 0 || n > h->dist_n) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->dist_n);
    for (int i = 0; i < n; ++i)
        if (!h->src[i].d_rgb.get())
            return fail(&h->err, IDC_ERR_UNSUPPORTED, "image slot %d has no resident source (idc_set_image_rgb with IDC_INGEST_KEEP_SOURCE)", i);
    for (int i = 0; i < n; ++i)
        if (h->src[i].gray_bits) return fail(&h->err, IDC_ERR_UNSUPPORTED, "image slot %d holds a greyscale source: it has no colour to score against", i);
    HIPCHK(h, hipSetDevice(h->device));
    rc = drain_pipeline(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    const size_t npix = (size_t)g.Hd * g.Wd, o_out = taps_align((size_t)g.B * 2 * sizeof(float));
    HIPCHK(h, h->d_score.ensure(o_out + lay.out_bytes, 65536));
    unsigned char* res = h->d_score.get() + o_out;
    HIPCHK(h, hipMemcpy(h->d_score.get(), centres, (size_t)g.B * 2 * sizeof(float), hipMemcpyHostToDevice));
    for (int i = 0; i < n; ++i) {
        const bool aa = h->src[i].d_net.get() != nullptr;       // the net-size image an antialiased ingestion made of this source
        HIPCHK(h, launch_dist_truth(aa ? h->src[i].d_net.get() : h->src[i].d_rgb.get(), nullptr, 1, aa ? h->H : h->src[i].h, aa ? h->W : h->src[i].w, h->H, h->W,
                                    g.s, (float*)(res + lay.o_truth) + (size_t)i * 2 * npix, h->stream.get()));
    }
    rc = launch_score(h, g, lay, (const float*)h->d_score.get(), res, h->stream.get());
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(out->xent, res + lay.o_xent, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (lay.ranks.n > 0) HIPCHK(h, hipMemcpy(out->hits, res + lay.o_hits, (size_t)n * lay.ranks.n * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (out->truth_ab) HIPCHK(h, hipMemcpy(out->truth_ab, res + lay.o_truth, (size_t)n * 2 * npix * sizeof(float), hipMemcpyDeviceToHost));
    if (out->xent_map) HIPCHK(h, hipMemcpy(out->xent_map, res + lay.o_xmap, (size_t)n * npix * sizeof(double), hipMemcpyDeviceToHost));
    if (out->rank_map) HIPCHK(h, hipMemcpy(out->rank_map, res + lay.o_rmap, (size_t)n * npix * sizeof(int), hipMemcpyDeviceToHost));
    if (out->target) HIPCHK(h, hipMemcpy(out->target, res + lay.o_tgt, (size_t)n * npix * sizeof(int), hipMemcpyDeviceToHost));
    return IDC_OK;
}

int idc_global_histogram(idc_handle h, int n, const uint8_t* rgb, const float* centres, float* hist, float* s_avg) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (n <= 0 || n > h->max_batch) return fail(&h->err, IDC_ERR_BATCH, "batch %d outside 1..%d", n, h->max_batch);
    if (!rgb || !centres || !hist) return fail(&h->err, IDC_ERR_INVALID_ARG, "null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure_post_buffers(h);                      // d_rgb doubles as the upload buffer of the reference image
    if (rc) return rc;
    const size_t hw = (size_t)h->H * h->W;
    DevMem<float> d_c; DevMem<unsigned> d_counts; DevMem<double> d_sat;
    HIPCHK(h, d_c.ensure(626 * 4)); HIPCHK(h, d_counts.ensure((size_t)n * 313 * 4)); HIPCHK(h, d_sat.ensure((size_t)n * 8));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, hipMemcpy(h->d_rgb.get(), rgb, (size_t)n * hw * 3, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d_c.get(), centres, 626 * 4, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemset(d_counts.get(), 0, (size_t)n * 313 * 4));
    HIPCHK(h, hipMemset(d_sat.get(), 0, (size_t)n * 8));
    HIPCHK(h, launch_global_stats(h->d_rgb.get(), d_c.get(), d_counts.get(), d_sat.get(), n, h->H, h->W, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    std::vector<unsigned> cnt((size_t)n * 313);
    std::vector<double> sat(n);
    HIPCHK(h, hipMemcpy(cnt.data(), d_counts.get(), cnt.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(sat.data(), d_sat.get(), (size_t)n * 8, hipMemcpyDeviceToHost));
    const double nblk = (double)(h->H / 4) * (h->W / 4);
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 313; ++k) hist[(size_t)i * 313 + k] = (float)(cnt[(size_t)i * 313 + k] / nblk);
        if (s_avg) s_avg[i] = (float)(sat[i] / (double)hw);
    }
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- reference-image global hints
// The blocking forms on the handle's own stage (check_refs / stage_refs / upload_refs / launch_refs: idc_exec.hip, shared with the pipelined
// slots).  Both end synchronised, so nothing of the stage is in flight when the next call grows it.
int idc_global_stats_rgb(idc_handle h, int m, const idc_ref_image* refs, const float* centres, float* hist, float* s_avg) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!hist) return fail(&h->err, IDC_ERR_INVALID_ARG, "null hist");
    RefLayout lay;
    int rc = check_refs(h, 1, 0, m, refs, nullptr, centres, 0.f, 0u, &lay);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    rc = drain_pipeline(h);
    if (rc) return rc;
    rc = stage_refs(h, h->ref, lay, refs, nullptr, centres, true);
    if (rc) return rc;
    rc = upload_refs(h, h->ref, lay, h->stream.get());
    if (rc) return rc;
    rc = launch_refs(h, h->ref, lay, 0.f, IDC_REF_SATURATION, nullptr, true, h->stream.get());
    if (rc) return rc;
    const size_t res_bytes = lay.o_savg - lay.o_hist + (size_t)m * sizeof(float);
    HIPCHK(h, hipMemcpyAsync(h->ref.h_res.get(), h->ref.d_work.get() + lay.o_hist, res_bytes, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    memcpy(hist, h->ref.h_res.get(), (size_t)m * 313 * sizeof(float));
    if (s_avg) memcpy(s_avg, h->ref.h_res.get() + (lay.o_savg - lay.o_hist), (size_t)m * sizeof(float));
    return IDC_OK;
}

int idc_set_global_refs(idc_handle h, int img, int n, int m, const idc_ref_image* refs, const int32_t* ref_index, const float* centres,
                        float hist_flag, unsigned flags) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!(h->flags & IDC_FLAG_GLOBAL_HINTS)) return fail(&h->err, IDC_ERR_UNSUPPORTED, "handle was created without IDC_FLAG_GLOBAL_HINTS");
    if (n < 1 || img < 0 || img >= h->max_batch || n > h->max_batch - img)
        return fail(&h->err, IDC_ERR_BATCH, "image slots %d..%d outside 0..%d", img, img + n - 1, h->max_batch - 1);
    RefLayout lay;
    int rc = check_refs(h, 1, n, m, refs, ref_index, centres, hist_flag, flags, &lay);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    rc = drain_pipeline(h);
    if (rc) return rc;
    rc = stage_refs(h, h->ref, lay, refs, ref_index, centres, false);
    if (rc) return rc;
    rc = upload_refs(h, h->ref, lay, h->stream.get());
    if (rc) return rc;
    rc = launch_refs(h, h->ref, lay, hist_flag, flags, h->d_glob_in.get() + (size_t)img * kGlobIn, false, h->stream.get());
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- stream ordering
// The handle's work runs on its own non-blocking stream.  A caller that produces device inputs or consumes device
// outputs on ANOTHER stream orders the two with these (or synchronises fully): wait = "the handle's stream waits for
// everything enqueued so far on caller_stream"; signal = "caller_stream waits for everything the handle enqueued so far".
int idc_stream_wait(idc_handle h, void* caller_stream) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventRecord(h->ev_sync.get(), (hipStream_t)caller_stream));
    HIPCHK(h, hipStreamWaitEvent(h->stream.get(), h->ev_sync.get(), 0));
    return IDC_OK;
}

int idc_stream_signal(idc_handle h, void* caller_stream) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventRecord(h->ev_sync.get(), h->stream.get()));
    HIPCHK(h, hipStreamWaitEvent((hipStream_t)caller_stream, h->ev_sync.get(), 0));
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- display step
// the resident [2,H,W] planes `source` names for image slot img (IDC_SRC_OUTPUT_AB: float64, *f64 = 1), or why they are not there
static int resident_ab_planes(idc_context* h, int img, int source, const void** pa, const void** pb, int* f64) {
    const size_t hw = (size_t)h->H * h->W;
    *f64 = 0;
    if (source == IDC_SRC_OUTPUT_AB) {
        if (!h->labq_resident || img >= h->last_n) return fail(&h->err, IDC_ERR_UNSUPPORTED, "no refreshed output_ab is resident (run idc_forward_rgb / idc_forward_resident with lab_q first)");
        *pa = h->d_labq.get() + ((size_t)img * 3 + 1) * hw; *pb = h->d_labq.get() + ((size_t)img * 3 + 2) * hw; *f64 = 1;
    } else if (source == IDC_SRC_OUTPUT_AB_RAW) {
        if (!h->out_resident || img >= h->last_n) return fail(&h->err, IDC_ERR_UNSUPPORTED, "no forward result is resident");
        *pa = h->d_out.get() + (size_t)img * 2 * hw; *pb = h->d_out.get() + ((size_t)img * 2 + 1) * hw;
    } else if (source == IDC_SRC_INPUT_AB) {
        *pa = h->d_ab.get() + (size_t)img * 2 * hw; *pb = h->d_ab.get() + ((size_t)img * 2 + 1) * hw;
    } else {
        return fail(&h->err, IDC_ERR_INVALID_ARG, "source %d not in 0..2", source);
    }
    return IDC_OK;
}

int idc_upsample_lab2rgb(idc_handle h, int img, int source, int interp, int out_h, int out_w, const double* L, uint8_t* rgb) {
    int rc = check_img(h, img);
    if (rc) return rc;
    if (!L || !rgb || out_h <= 0 || out_w <= 0) return fail(&h->err, IDC_ERR_INVALID_ARG, "bad output geometry / null pointer");
    if (interp < 0 || interp > 2) return fail(&h->err, IDC_ERR_INVALID_ARG, "interp %d not in 0..2", interp);
    HIPCHK(h, hipSetDevice(h->device));
    const void *pa = nullptr, *pb = nullptr; int f64 = 0;
    rc = resident_ab_planes(h, img, source, &pa, &pb, &f64);
    if (rc) return rc;
    rc = drain_pipeline(h);
    if (rc) return rc;
    const size_t np = (size_t)out_h * out_w;
    if (h->d_up_rgb.bytes() < np * 3 || h->d_up_L.bytes() < np * 8 || h->h_up_rgb.bytes() < np * 3 || h->h_up_L.bytes() < np * 8)
        HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    HIPCHK(h, h->d_up_rgb.ensure(np * 3));
    HIPCHK(h, h->d_up_L.ensure(np * 8));
    HIPCHK(h, h->h_up_rgb.ensure(np * 3));
    HIPCHK(h, h->h_up_L.ensure(np * 8));
    memcpy(h->h_up_L.get(), L, np * 8);
    HIPCHK(h, hipMemcpyAsync(h->d_up_L.get(), h->h_up_L.get(), np * 8, hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, launch_upsample_lab2rgb(pa, pb, f64, h->H, h->W, interp, (const double*)h->d_up_L.get(), out_h, out_w, h->d_up_rgb.get(), h->stream.get()));
    HIPCHK(h, hipMemcpyAsync(h->h_up_rgb.get(), h->d_up_rgb.get(), np * 3, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    memcpy(rgb, h->h_up_rgb.get(), np * 3);
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- image ingestion
static int ensure_ingest_buffers(idc_context* h) {
    const size_t hw = (size_t)h->H * h->W, nb = (size_t)h->max_batch;
    HIPCHK(h, h->d_src_ptrs.ensure(nb * sizeof(void*)));
    HIPCHK(h, h->h_src_ptrs.ensure(nb * sizeof(void*)));
    HIPCHK(h, h->d_net_lab.ensure(nb * hw * 3 * 8));
    HIPCHK(h, h->d_net_rgb.ensure(nb * hw * 3));
    return IDC_OK;
}

// The antialiased pre-pass of a blocking ingestion (the filter is on and the n sources of src_h x src_w are down-scaled: the caller checked).
// h_src_ptrs[0..n) name the sources on the device, uploaded or on their way on the handle's stream; on return they name the net-size lattice
// images [H,W,channels] the pre-pass writes instead -- a kept source's in its slot, the others in the handle's scratch -- for the ingestion
// kernel to read at source size (H, W).  Nothing of the previous call is in flight (the caller synchronised), so the buffers may grow.
static int antialias_sources(idc_context* h, int img, int n, int src_h, int src_w, int bits, int channels, bool keep) {
    const size_t net_bytes = (size_t)h->H * h->W * channels * (size_t)(bits / 8);
    HIPCHK(h, h->d_aa_jobs.ensure((size_t)h->max_batch * sizeof(ResampleJob)));
    HIPCHK(h, h->h_aa_jobs.ensure((size_t)h->max_batch * sizeof(ResampleJob)));
    if (!keep) HIPCHK(h, h->d_aa.ensure((size_t)n * net_bytes));
    ResampleJob* jobs = (ResampleJob*)h->h_aa_jobs.get();
    int tiles = 0;
    for (int i = 0; i < n; ++i) {
        unsigned char* dst = nullptr;
        if (keep) {
            HIPCHK(h, h->src[img + i].d_net.ensure(net_bytes));
            dst = h->src[img + i].d_net.get();
        } else {
            dst = h->d_aa.get() + (size_t)i * net_bytes;
        }
        jobs[i] = resample_job((long long)(uintptr_t)h->h_src_ptrs.get()[i], (long long)(uintptr_t)dst, src_h, src_w, h->W, channels);
        tiles = tiles > jobs[i].tiles ? tiles : jobs[i].tiles;
        h->h_src_ptrs.get()[i] = dst;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_aa_jobs.get(), jobs, (size_t)n * sizeof(ResampleJob), hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, launch_resample(nullptr, nullptr, (const ResampleJob*)h->d_aa_jobs.get(), n, tiles, bits, channels, h->H, h->W, h->stream.get()));
    return IDC_OK;
}

int idc_set_image_rgb(idc_handle h, int img, int n, int src_h, int src_w, const uint8_t* rgb, float l_cent, unsigned flags,
                      uint8_t* rgb_net, double* lab_net) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (!rgb) return fail(&h->err, IDC_ERR_INVALID_ARG, "null rgb");
    if (flags & ~(unsigned)IDC_INGEST_KEEP_SOURCE) return fail(&h->err, IDC_ERR_INVALID_ARG, "unknown flag bits 0x%x", flags);
    if (src_h < 1 || src_h > 16384 || src_w < 1 || src_w > 16384)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "source size %dx%d outside 1..16384", src_h, src_w);
    if (n < 1 || img < 0 || img >= h->max_batch || n > h->max_batch - img)
        return fail(&h->err, IDC_ERR_BATCH, "image slots %d..%d outside 0..%d", img, img + n - 1, h->max_batch - 1);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain_pipeline(h);
    if (rc) return rc;
    rc = ensure_ingest_buffers(h);
    if (rc) return rc;
    const size_t hw = (size_t)h->H * h->W, sb = (size_t)src_h * src_w * 3;
    const bool keep = (flags & IDC_INGEST_KEEP_SOURCE) != 0;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));            // the pointer table and the upload buffer of the previous call may still be read
    for (int i = 0; i < n; ++i) drop_source(h, img + i);   // a slot's previous source goes either way; a kept one gets its own allocation
    if (keep) {
        for (int i = 0; i < n; ++i) {
            auto& sl = h->src[img + i];
            HIPCHK(h, sl.d_rgb.ensure(sb));
            sl.h = src_h; sl.w = src_w; sl.l_cent = l_cent;
            h->h_src_ptrs.get()[i] = sl.d_rgb.get();
        }
    } else {
        HIPCHK(h, h->d_ingest.ensure((size_t)n * sb));
        for (int i = 0; i < n; ++i) h->h_src_ptrs.get()[i] = h->d_ingest.get() + (size_t)i * sb;
    }
    const bool in_pinned = is_pinned(rgb);                 // pinned: transferred in place on the stream; pageable: the runtime stages it
    for (int i = 0; i < n; ++i) {
        void* dst = (void*)h->h_src_ptrs.get()[i];
        if (in_pinned) HIPCHK(h, hipMemcpyAsync(dst, rgb + (size_t)i * sb, sb, hipMemcpyHostToDevice, h->stream.get()));
        else HIPCHK(h, hipMemcpy(dst, rgb + (size_t)i * sb, sb, hipMemcpyHostToDevice));
    }
    const bool aa = h->ingest_filter == IDC_FILTER_ANTIALIAS && resample_applies(src_h, src_w, h->H, h->W);
    if (aa) {
        rc = antialias_sources(h, img, n, src_h, src_w, 8, 3, keep);
        if (rc) return rc;
    }
    HIPCHK(h, hipMemcpyAsync((void*)h->d_src_ptrs.get(), (const void*)h->h_src_ptrs.get(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, launch_ingest(0, (const void* const*)h->d_src_ptrs.get(), n, aa ? h->H : src_h, aa ? h->W : src_w, h->H, h->W, l_cent, h->d_L.get() + (size_t)img * hw,
                            rgb_net ? h->d_net_rgb.get() : nullptr, lab_net ? h->d_net_lab.get() : nullptr, h->stream.get()));
    const bool rgb_direct = rgb_net && is_pinned(rgb_net), lab_direct = lab_net && is_pinned(lab_net);
    if (rgb_direct) HIPCHK(h, hipMemcpyAsync(rgb_net, h->d_net_rgb.get(), (size_t)n * hw * 3, hipMemcpyDeviceToHost, h->stream.get()));
    if (lab_direct) HIPCHK(h, hipMemcpyAsync(lab_net, h->d_net_lab.get(), (size_t)n * hw * 3 * 8, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    if (rgb_net && !rgb_direct) HIPCHK(h, hipMemcpy(rgb_net, h->d_net_rgb.get(), (size_t)n * hw * 3, hipMemcpyDeviceToHost));
    if (lab_net && !lab_direct) HIPCHK(h, hipMemcpy(lab_net, h->d_net_lab.get(), (size_t)n * hw * 3 * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) h->l_set[img + i] = 1;
    return IDC_OK;
}

// idc_set_image_rgb for n planes [src_h,src_w] of uint8 (bits 8) or uint16 (bits 16): the same steps with the sample as the unit.  The net-size
// plane and its L leave through the buffers of idc_set_image_rgb's results, which are large enough for either width.
int idc_set_image_gray(idc_handle h, int img, int n, int src_h, int src_w, int bits, const void* pix, float l_cent, unsigned flags, void* gray_net,
                       double* l_net) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (bits != 8 && bits != 16) return fail(&h->err, IDC_ERR_INVALID_ARG, "bits %d is neither 8 nor 16", bits);
    if (!pix) return fail(&h->err, IDC_ERR_INVALID_ARG, "null pix");
    if (bits == 16 && (((uintptr_t)pix | (uintptr_t)gray_net) & 1)) return fail(&h->err, IDC_ERR_INVALID_ARG, "16-bit samples at an odd address");
    if (flags & ~(unsigned)IDC_INGEST_KEEP_SOURCE) return fail(&h->err, IDC_ERR_INVALID_ARG, "unknown flag bits 0x%x", flags);
    if (src_h < 1 || src_h > 16384 || src_w < 1 || src_w > 16384)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "source size %dx%d outside 1..16384", src_h, src_w);
    if (n < 1 || img < 0 || img >= h->max_batch || n > h->max_batch - img)
        return fail(&h->err, IDC_ERR_BATCH, "image slots %d..%d outside 0..%d", img, img + n - 1, h->max_batch - 1);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain_pipeline(h);
    if (rc) return rc;
    rc = ensure_ingest_buffers(h);
    if (rc) return rc;
    const size_t hw = (size_t)h->H * h->W, sz = (size_t)bits / 8, sb = (size_t)src_h * src_w * sz;
    const bool keep = (flags & IDC_INGEST_KEEP_SOURCE) != 0;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));            // the pointer table and the upload buffer of the previous call may still be read
    for (int i = 0; i < n; ++i) drop_source(h, img + i);
    if (keep) {
        for (int i = 0; i < n; ++i) {
            auto& sl = h->src[img + i];
            HIPCHK(h, sl.d_rgb.ensure(sb));
            sl.h = src_h; sl.w = src_w; sl.l_cent = l_cent; sl.gray_bits = bits;
            h->h_src_ptrs.get()[i] = sl.d_rgb.get();
        }
    } else {
        HIPCHK(h, h->d_ingest.ensure((size_t)n * ((sb + 3) & ~(size_t)3)));
        for (int i = 0; i < n; ++i) h->h_src_ptrs.get()[i] = h->d_ingest.get() + (size_t)i * ((sb + 3) & ~(size_t)3);     // a uint16 plane starts even
    }
    const unsigned char* in = (const unsigned char*)pix;
    const bool in_pinned = is_pinned(pix);
    for (int i = 0; i < n; ++i) {
        void* dst = (void*)h->h_src_ptrs.get()[i];
        if (in_pinned) HIPCHK(h, hipMemcpyAsync(dst, in + (size_t)i * sb, sb, hipMemcpyHostToDevice, h->stream.get()));
        else HIPCHK(h, hipMemcpy(dst, in + (size_t)i * sb, sb, hipMemcpyHostToDevice));
    }
    const bool aa = h->ingest_filter == IDC_FILTER_ANTIALIAS && resample_applies(src_h, src_w, h->H, h->W);
    if (aa) {
        rc = antialias_sources(h, img, n, src_h, src_w, bits, 1, keep);
        if (rc) return rc;
    }
    HIPCHK(h, hipMemcpyAsync((void*)h->d_src_ptrs.get(), (const void*)h->h_src_ptrs.get(), (size_t)n * sizeof(void*), hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, launch_ingest(bits, (const void* const*)h->d_src_ptrs.get(), n, aa ? h->H : src_h, aa ? h->W : src_w, h->H, h->W, l_cent, h->d_L.get() + (size_t)img * hw,
                            gray_net ? h->d_net_rgb.get() : nullptr, l_net ? h->d_net_lab.get() : nullptr, h->stream.get()));
    const bool net_direct = gray_net && is_pinned(gray_net), l_direct = l_net && is_pinned(l_net);
    if (net_direct) HIPCHK(h, hipMemcpyAsync(gray_net, h->d_net_rgb.get(), (size_t)n * hw * sz, hipMemcpyDeviceToHost, h->stream.get()));
    if (l_direct) HIPCHK(h, hipMemcpyAsync(l_net, h->d_net_lab.get(), (size_t)n * hw * 8, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    if (gray_net && !net_direct) HIPCHK(h, hipMemcpy(gray_net, h->d_net_rgb.get(), (size_t)n * hw * sz, hipMemcpyDeviceToHost));
    if (l_net && !l_direct) HIPCHK(h, hipMemcpy(l_net, h->d_net_lab.get(), (size_t)n * hw * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) h->l_set[img + i] = 1;
    return IDC_OK;
}

// idc_fullres_rgb / idc_fullres_rgb16 (rgb; out_bits 8 | 16) and idc_fullres_ab (ab): one list of checks, one residency rule.  A kept greyscale
// source (SlotSource::gray_bits) is served by the grey kernels.
// ycc_format != IDC_OUT_RGB (idc_fullres_ycc): rgb receives the image's plane block, made from the RGB result where the kernels below left it.
static int fullres(idc_handle h, int img, int source, int interp, int l_mode, void* rgb, int out_bits, double* ab, bool want_ab,
                   int ycc_format = IDC_OUT_RGB, int ycc_matrix = IDC_YCC_JFIF) {
    int rc = check_img(h, img);
    if (rc) return rc;
    if (interp < 0 || interp > IDC_INTERP_JOINT) return fail(&h->err, IDC_ERR_INVALID_ARG, "interp %d not in 0..3", interp);
    if (l_mode != IDC_L_IMAGE && l_mode != IDC_L_MASK50) return fail(&h->err, IDC_ERR_INVALID_ARG, "l_mode %d not in 0..1", l_mode);
    if (interp == IDC_INTERP_JOINT && l_mode != IDC_L_IMAGE)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "IDC_INTERP_JOINT is guided by the L of the source pixels: it needs IDC_L_IMAGE");
    if (source < IDC_SRC_OUTPUT_AB || source > IDC_SRC_NO_AB) return fail(&h->err, IDC_ERR_INVALID_ARG, "source %d not in 0..3", source);
    const auto& sl = h->src[img];
    if (!sl.d_rgb.get()) return fail(&h->err, IDC_ERR_UNSUPPORTED, "image slot %d has no resident source (idc_set_image_rgb with IDC_INGEST_KEEP_SOURCE)", img);
    if (want_ab ? !ab : !rgb) return fail(&h->err, IDC_ERR_INVALID_ARG, want_ab ? "null ab" : "null rgb");
    HIPCHK(h, hipSetDevice(h->device));
    const void *pa = nullptr, *pb = nullptr; int f64 = 0;
    if (source != IDC_SRC_NO_AB) {
        rc = resident_ab_planes(h, img, source, &pa, &pb, &f64);
        if (rc) return rc;
    }
    rc = drain_pipeline(h);
    if (rc) return rc;
    const size_t hw = (size_t)h->H * h->W;
    if (want_ab) {
        const size_t nbytes = (size_t)sl.h * sl.w * 2 * sizeof(double);
        const bool direct = is_pinned(ab);
        if (h->d_full_ab.bytes() < nbytes) {
            HIPCHK(h, hipStreamSynchronize(h->stream.get()));
            HIPCHK(h, h->d_full_ab.ensure(nbytes));
        }
        if (!direct) HIPCHK(h, h->h_full_ab.ensure(h->d_full_ab.bytes()));
        HIPCHK(h, launch_joint_fullres(sl.gray_bits, sl.d_rgb.get(), nullptr, 1, sl.h, sl.w, joint_tiles(sl.h, sl.w), pa, pb, f64, 0,
                                       h->d_L.get() + (size_t)img * hw, sl.l_cent, h->H, h->W, interp, h->joint, nullptr, 8, h->d_full_ab.get(),
                                       h->stream.get()));
        HIPCHK(h, hipMemcpyAsync(direct ? ab : h->h_full_ab.get(), h->d_full_ab.get(), nbytes, hipMemcpyDeviceToHost, h->stream.get()));
        HIPCHK(h, hipStreamSynchronize(h->stream.get()));
        if (!direct) memcpy(ab, h->h_full_ab.get(), nbytes);
        return IDC_OK;
    }
    const size_t nbytes = (size_t)sl.h * sl.w * 3 * (size_t)(out_bits / 8);
    const bool direct = is_pinned(rgb);                    // a pinned result buffer is written in place; a pageable one through pinned staging
    if (h->d_full_rgb.bytes() < nbytes) {
        HIPCHK(h, hipStreamSynchronize(h->stream.get()));
        HIPCHK(h, h->d_full_rgb.ensure(nbytes));
    }
    if (!direct && ycc_format == IDC_OUT_RGB) HIPCHK(h, h->h_full_rgb.ensure(h->d_full_rgb.bytes()));
    const float* mask = l_mode == IDC_L_MASK50 ? h->d_mask.get() + (size_t)img * hw : nullptr;
    if (interp == IDC_INTERP_JOINT && pa)
        HIPCHK(h, launch_joint_fullres(sl.gray_bits, sl.d_rgb.get(), nullptr, 1, sl.h, sl.w, joint_tiles(sl.h, sl.w), pa, pb, f64, 0,
                                       h->d_L.get() + (size_t)img * hw, sl.l_cent, h->H, h->W, interp, h->joint, h->d_full_rgb.get(), out_bits, nullptr,
                                       h->stream.get()));
    else        // (IDC_SRC_NO_AB has nothing to interpolate: a = b = 0 whatever the interp)
        HIPCHK(h, launch_fullres(sl.gray_bits, sl.d_rgb.get(), sl.h, sl.w, pa, pb, f64, h->H, h->W, interp == IDC_INTERP_JOINT ? IDC_INTERP_LINEAR : interp,
                                 mask, h->hint_mask_value[img], h->d_full_rgb.get(), out_bits, h->stream.get()));
    if (ycc_format != IDC_OUT_RGB) {      // the post-pass on the one image, and its block instead of the RGB
        const size_t yb = ycc420_bytes(sl.h, sl.w);
        HIPCHK(h, hipStreamSynchronize(h->stream.get()));            // the table of the previous call may still be in flight
        HIPCHK(h, h->d_ycc.ensure(yb, 65536));
        HIPCHK(h, h->d_ycc_meta.ensure(sizeof(YccDesc), 4096));
        HIPCHK(h, h->h_ycc_meta.ensure(sizeof(YccDesc), 4096));
        if (!direct) HIPCHK(h, h->h_ycc.ensure(h->d_ycc.bytes()));
        const YccDesc d = {0, 0, sl.h, sl.w};
        memcpy(h->h_ycc_meta.get(), &d, sizeof(d));
        HIPCHK(h, hipMemcpyAsync(h->d_ycc_meta.get(), h->h_ycc_meta.get(), sizeof(d), hipMemcpyHostToDevice, h->stream.get()));
        HIPCHK(h, launch_ycc420(h->d_full_rgb.get(), (const YccDesc*)h->d_ycc_meta.get(), 1, ycc_blocks(sl.h, sl.w), ycc_format, ycc_matrix,
                                h->d_ycc.get(), h->stream.get()));
        HIPCHK(h, hipMemcpyAsync(direct ? rgb : h->h_ycc.get(), h->d_ycc.get(), yb, hipMemcpyDeviceToHost, h->stream.get()));
        HIPCHK(h, hipStreamSynchronize(h->stream.get()));
        if (!direct) memcpy(rgb, h->h_ycc.get(), yb);
        return IDC_OK;
    }
    HIPCHK(h, hipMemcpyAsync(direct ? rgb : h->h_full_rgb.get(), h->d_full_rgb.get(), nbytes, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    if (!direct) memcpy(rgb, h->h_full_rgb.get(), nbytes);
    return IDC_OK;
}

int idc_fullres_rgb(idc_handle h, int img, int source, int interp, int l_mode, uint8_t* rgb) {
    return fullres(h, img, source, interp, l_mode, rgb, 8, nullptr, false);
}

int idc_fullres_rgb16(idc_handle h, int img, int source, int interp, uint16_t* rgb) {
    int rc = check_img(h, img);
    if (rc) return rc;
    if (!h->src[img].d_rgb.get() || h->src[img].gray_bits != 16)
        return fail(&h->err, IDC_ERR_UNSUPPORTED, "image slot %d has no resident 16-bit greyscale source (idc_set_image_gray with bits 16 and IDC_INGEST_KEEP_SOURCE)", img);
    if (!rgb || ((uintptr_t)rgb & 1)) return fail(&h->err, IDC_ERR_INVALID_ARG, rgb ? "rgb at an odd address" : "null rgb");
    return fullres(h, img, source, interp, IDC_L_IMAGE, rgb, 16, nullptr, false);
}

int idc_fullres_ab(idc_handle h, int img, int source, int interp, double* ab) {
    return fullres(h, img, source, interp, IDC_L_IMAGE, nullptr, 8, ab, true);
}

int idc_set_joint_upsample(idc_handle h, int radius, double sigma_s, double sigma_r) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (radius < 1 || radius > 4) return fail(&h->err, IDC_ERR_INVALID_ARG, "radius %d outside 1..4", radius);
    if (!(sigma_s >= 0.25 && sigma_s <= 8.0)) return fail(&h->err, IDC_ERR_INVALID_ARG, "sigma_s %g outside 0.25..8", sigma_s);
    if (!(sigma_r >= 0.5 && sigma_r <= 100.0)) return fail(&h->err, IDC_ERR_INVALID_ARG, "sigma_r %g outside 0.5..100", sigma_r);
    h->joint = {radius, 2.0 * sigma_s * sigma_s, 2.0 * sigma_r * sigma_r};
    return IDC_OK;
}

int idc_set_batch_upsample(idc_handle h, int interp) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (interp != IDC_INTERP_LINEAR && interp != IDC_INTERP_JOINT)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "interp %d is neither IDC_INTERP_LINEAR nor IDC_INTERP_JOINT", interp);
    h->batch_interp = interp;
    return IDC_OK;
}

int idc_set_ingest_filter(idc_handle h, int filter) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (filter != IDC_FILTER_BILINEAR && filter != IDC_FILTER_ANTIALIAS)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "filter %d is neither IDC_FILTER_BILINEAR nor IDC_FILTER_ANTIALIAS", filter);
    h->ingest_filter = filter;
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- YCbCr 4:2:0 output
static bool ycc_format_ok(int format) { return format == IDC_OUT_I420 || format == IDC_OUT_NV12; }
static bool ycc_matrix_ok(int matrix) { return matrix == IDC_YCC_JFIF || matrix == IDC_YCC_BT709_VIDEO; }

size_t idc_ycc420_bytes(int h, int w) { return ycc420_bytes(h, w); }

int idc_set_batch_output(idc_handle h, int format, int matrix) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (format != IDC_OUT_RGB && !ycc_format_ok(format))
        return fail(&h->err, IDC_ERR_INVALID_ARG, "format %d is none of IDC_OUT_RGB, IDC_OUT_I420, IDC_OUT_NV12", format);
    if (!ycc_matrix_ok(matrix)) return fail(&h->err, IDC_ERR_INVALID_ARG, "matrix %d is neither IDC_YCC_JFIF nor IDC_YCC_BT709_VIDEO", matrix);
    h->out_format = format; h->out_matrix = matrix;
    return IDC_OK;
}

int idc_fullres_ycc(idc_handle h, int img, int source, int interp, int l_mode, int format, int matrix, uint8_t* out) {
    int rc = check_img(h, img);
    if (rc) return rc;
    if (!ycc_format_ok(format)) return fail(&h->err, IDC_ERR_INVALID_ARG, "format %d is neither IDC_OUT_I420 nor IDC_OUT_NV12", format);
    if (!ycc_matrix_ok(matrix)) return fail(&h->err, IDC_ERR_INVALID_ARG, "matrix %d is neither IDC_YCC_JFIF nor IDC_YCC_BT709_VIDEO", matrix);
    return fullres(h, img, source, interp, l_mode, out, 8, nullptr, false, format, matrix);
}

// The conversion alone: the images packed back to back into one upload, one launch, the blocks packed back to back into one copy back
int idc_rgb_to_ycc420(idc_handle h, int n, const idc_ref_image* images, int format, int matrix, uint8_t* const* out) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (n < 1 || n > IDC_REF_MAX) return fail(&h->err, IDC_ERR_BATCH, "%d images outside 1..%d", n, IDC_REF_MAX);
    if (!images || !out) return fail(&h->err, IDC_ERR_INVALID_ARG, "null image table");
    if (!ycc_format_ok(format)) return fail(&h->err, IDC_ERR_INVALID_ARG, "format %d is neither IDC_OUT_I420 nor IDC_OUT_NV12", format);
    if (!ycc_matrix_ok(matrix)) return fail(&h->err, IDC_ERR_INVALID_ARG, "matrix %d is neither IDC_YCC_JFIF nor IDC_YCC_BT709_VIDEO", matrix);
    size_t in_bytes = 0, out_bytes = 0;
    int max_blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (!images[i].rgb || !out[i]) return fail(&h->err, IDC_ERR_INVALID_ARG, "image %d: null pointer", i);
        if (images[i].h < 1 || images[i].h > kYccMaxSide || images[i].w < 1 || images[i].w > kYccMaxSide)
            return fail(&h->err, IDC_ERR_INVALID_ARG, "image %d: size %dx%d outside 1..%d", i, images[i].h, images[i].w, kYccMaxSide);
        in_bytes += (size_t)images[i].h * images[i].w * 3;
        out_bytes += ycc420_bytes(images[i].h, images[i].w);
        max_blocks = max_blocks > ycc_blocks(images[i].h, images[i].w) ? max_blocks : ycc_blocks(images[i].h, images[i].w);
    }
    if (in_bytes > IDC_BATCH_MAX_SOURCE_BYTES)
        return fail(&h->err, IDC_ERR_INVALID_ARG, "%d images hold %zu bytes, more than %zu", n, in_bytes, (size_t)IDC_BATCH_MAX_SOURCE_BYTES);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = drain_pipeline(h);
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));                // the buffers of the previous call may still be in flight
    const size_t meta_bytes = (size_t)n * sizeof(YccDesc);
    HIPCHK(h, h->d_ycc_in.ensure(in_bytes, 65536));
    HIPCHK(h, h->h_ycc_in.ensure(in_bytes, 65536));
    HIPCHK(h, h->d_ycc.ensure(out_bytes, 65536));
    HIPCHK(h, h->h_ycc.ensure(h->d_ycc.bytes()));
    HIPCHK(h, h->d_ycc_meta.ensure(meta_bytes, 4096));
    HIPCHK(h, h->h_ycc_meta.ensure(meta_bytes, 4096));
    YccDesc* tab = (YccDesc*)h->h_ycc_meta.get();
    size_t src = 0, dst = 0;
    for (int i = 0; i < n; ++i) {
        const size_t sb = (size_t)images[i].h * images[i].w * 3;
        tab[i].src = (long long)src; tab[i].dst = (long long)dst; tab[i].h = images[i].h; tab[i].w = images[i].w;
        memcpy(h->h_ycc_in.get() + src, images[i].rgb, sb);
        src += sb; dst += ycc420_bytes(images[i].h, images[i].w);
    }
    HIPCHK(h, hipMemcpyAsync(h->d_ycc_meta.get(), h->h_ycc_meta.get(), meta_bytes, hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, hipMemcpyAsync(h->d_ycc_in.get(), h->h_ycc_in.get(), in_bytes, hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, launch_ycc420(h->d_ycc_in.get(), (const YccDesc*)h->d_ycc_meta.get(), n, max_blocks, format, matrix, h->d_ycc.get(), h->stream.get()));
    // a pinned destination is written in place, the pageable ones through the pinned twin: neighbouring pageable blocks as one copy
    size_t run0 = 0, run1 = 0;
    for (int i = 0; i <= n; ++i) {
        const bool direct = i < n && is_pinned(out[i]);
        if (i == n || direct) {
            if (run1 != run0) HIPCHK(h, hipMemcpyAsync(h->h_ycc.get() + run0, h->d_ycc.get() + run0, run1 - run0, hipMemcpyDeviceToHost, h->stream.get()));
            if (i == n) break;
            HIPCHK(h, hipMemcpyAsync(out[i], h->d_ycc.get() + (size_t)tab[i].dst, ycc420_bytes(tab[i].h, tab[i].w), hipMemcpyDeviceToHost, h->stream.get()));
            run0 = run1 = (size_t)tab[i].dst + ycc420_bytes(tab[i].h, tab[i].w);
        } else {
            run1 = (size_t)tab[i].dst + ycc420_bytes(tab[i].h, tab[i].w);
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    for (int i = 0; i < n; ++i)
        if (!is_pinned(out[i])) memcpy(out[i], h->h_ycc.get() + (size_t)tab[i].dst, ycc420_bytes(tab[i].h, tab[i].w));
    return IDC_OK;
}

// ---------------------------------------------------------------------------------------------- colour picker
// One device and one pinned buffer carry a call's inputs and results; both calls block, so nothing of the previous call is in flight when they grow
static int ensure_pick_buffers(idc_context* h, size_t bytes) {
    HIPCHK(h, h->d_pick.ensure(bytes, 65536));
    HIPCHK(h, h->h_pick.ensure(bytes, 65536));
    return IDC_OK;
}

static int check_pick_L(idc_context* h, int n, const double* L) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(L[k])) return fail(&h->err, IDC_ERR_INVALID_ARG, "L[%d] is not finite", k);
    return IDC_OK;
}

int idc_gamut_map(idc_handle h, int n, const double* L, int gamut_size, int D, uint8_t* pts_rgb, uint8_t* masked_rgb, uint8_t* mask) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (n < 1 || n > IDC_GAMUT_MAX_MAPS) return fail(&h->err, IDC_ERR_INVALID_ARG, "%d maps outside 1..%d", n, IDC_GAMUT_MAX_MAPS);
    if (!L) return fail(&h->err, IDC_ERR_INVALID_ARG, "null L");
    if (gamut_size < 1 || gamut_size > IDC_GAMUT_MAX_SIZE) return fail(&h->err, IDC_ERR_INVALID_ARG, "gamut_size %d outside 1..%d", gamut_size, IDC_GAMUT_MAX_SIZE);
    if (D < 1 || D > gamut_size) return fail(&h->err, IDC_ERR_INVALID_ARG, "D %d outside 1..gamut_size (%d)", D, gamut_size);
    if (!pts_rgb && !masked_rgb && !mask) return fail(&h->err, IDC_ERR_INVALID_ARG, "every output is null");
    int rc = check_pick_L(h, n, L);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const int A = (2 * gamut_size + D - 1) / D + 1;        // len(arange(-gamut_size, gamut_size + D, D))
    const size_t in_bytes = (size_t)n * 8, np = (size_t)n * A * A;
    const size_t o_pts = in_bytes, o_masked = o_pts + (pts_rgb ? np * 3 : 0), o_mask = o_masked + (masked_rgb ? np * 3 : 0);
    const size_t total = o_mask + (mask ? np : 0);
    rc = ensure_pick_buffers(h, total);
    if (rc) return rc;
    memcpy(h->h_pick.get(), L, in_bytes);
    HIPCHK(h, hipMemcpyAsync(h->d_pick.get(), h->h_pick.get(), in_bytes, hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, launch_gamut_map((const double*)h->d_pick.get(), n, gamut_size, D, A, pts_rgb ? h->d_pick.get() + o_pts : nullptr,
                               masked_rgb ? h->d_pick.get() + o_masked : nullptr, mask ? h->d_pick.get() + o_mask : nullptr, h->stream.get()));
    HIPCHK(h, hipMemcpyAsync(h->h_pick.get() + in_bytes, h->d_pick.get() + in_bytes, total - in_bytes, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    if (pts_rgb) memcpy(pts_rgb, h->h_pick.get() + o_pts, np * 3);
    if (masked_rgb) memcpy(masked_rgb, h->h_pick.get() + o_masked, np * 3);
    if (mask) memcpy(mask, h->h_pick.get() + o_mask, np);
    return IDC_OK;
}

int idc_snap_colors(idc_handle h, int n, const double* L, const uint8_t* rgb, uint8_t* rgb_out, double* lab_out, int32_t* iters) {
    if (!h) return fail(nullptr, IDC_ERR_INVALID_ARG, "null handle");
    if (n < 1 || n > IDC_SNAP_MAX_COLORS) return fail(&h->err, IDC_ERR_INVALID_ARG, "%d colours outside 1..%d", n, IDC_SNAP_MAX_COLORS);
    if (!L || !rgb) return fail(&h->err, IDC_ERR_INVALID_ARG, "null L or rgb");
    if (!rgb_out && !lab_out && !iters) return fail(&h->err, IDC_ERR_INVALID_ARG, "every output is null");
    int rc = check_pick_L(h, n, L);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    // [L n f64][rgb n*3 u8, padded to 8][lab_out n*3 f64][iters n i32][rgb_out n*3 u8]: inputs first, every section aligned for its type
    const size_t nn = (size_t)n, o_rgb = nn * 8, in_bytes = o_rgb + ((nn * 3 + 7) & ~(size_t)7);
    const size_t o_lab = in_bytes, o_it = o_lab + (lab_out ? nn * 24 : 0), o_out = o_it + (iters ? nn * 4 : 0);
    const size_t total = o_out + (rgb_out ? nn * 3 : 0);
    rc = ensure_pick_buffers(h, total);
    if (rc) return rc;
    memcpy(h->h_pick.get(), L, nn * 8);
    memcpy(h->h_pick.get() + o_rgb, rgb, nn * 3);
    HIPCHK(h, hipMemcpyAsync(h->d_pick.get(), h->h_pick.get(), in_bytes, hipMemcpyHostToDevice, h->stream.get()));
    HIPCHK(h, launch_snap_colors((const double*)h->d_pick.get(), h->d_pick.get() + o_rgb, n, rgb_out ? h->d_pick.get() + o_out : nullptr,
                                 lab_out ? (double*)(h->d_pick.get() + o_lab) : nullptr, iters ? (int*)(h->d_pick.get() + o_it) : nullptr, h->stream.get()));
    HIPCHK(h, hipMemcpyAsync(h->h_pick.get() + in_bytes, h->d_pick.get() + in_bytes, total - in_bytes, hipMemcpyDeviceToHost, h->stream.get()));
    HIPCHK(h, hipStreamSynchronize(h->stream.get()));
    if (lab_out) memcpy(lab_out, h->h_pick.get() + o_lab, nn * 24);
    if (iters) memcpy(iters, h->h_pick.get() + o_it, nn * 4);
    if (rgb_out) memcpy(rgb_out, h->h_pick.get() + o_out, nn * 3);
    return IDC_OK;
}

void* idc_stream(idc_handle h) { return h ? (void*)h->stream.get() : nullptr; }

}  // extern "C"
