// idc_batch.h -- the plan of one pipelined batch (idc_forward_async_rgb and its five relatives, idc_exec.hip): what a call passes, every check
// of its arguments that needs neither the handle's state nor the runtime, the byte layout of what travels, and which copies move it.  Host
// code that makes no runtime call: tools/batch_selftest.cpp includes it alone and checks the layouts without a device.
#ifndef IDC_BATCH_H
#define IDC_BATCH_H

#include <stdarg.h>
#include <stdio.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/ideepcolor.h"
#include "idc_kernels.h"

namespace idc {

// cv2.rectangle, as every hint list is read: corners in either order, inclusive, clipped to the H x W net size.  false = entirely outside
// the image (r is filled all the same).
inline bool clip_hint(const idc_hint& u, int H, int W, HintRect& r) {
    r.y0 = u.y0 < u.y1 ? u.y0 : u.y1; r.y1 = u.y0 < u.y1 ? u.y1 : u.y0;
    r.x0 = u.x0 < u.x1 ? u.x0 : u.x1; r.x1 = u.x0 < u.x1 ? u.x1 : u.x0;
    if (r.y0 < 0) r.y0 = 0;
    if (r.x0 < 0) r.x0 = 0;
    if (r.y1 > H - 1) r.y1 = H - 1;
    if (r.x1 > W - 1) r.x1 = W - 1;
    r.c0 = u.c0; r.c1 = u.c1; r.c2 = u.c2;
    return r.y0 <= r.y1 && r.x0 <= r.x1;
}

// What the six entry points pass.  The same-size calls: ONE array each way, [n,src_h,src_w,3] in and [n,H,W,3] or [n,src_h,src_w,3] out.
// ragged (idc_forward_async_images and later): a descriptor and an output pointer per image; on the device the sources and the source-size
// results lie packed back to back, the layout the same-size calls have anyway, so everything but the two colour kernels is shared.
struct BatchCall {
    int slot = 0, n = 0;
    bool ragged = false;
    int src_h = 0, src_w = 0; const uint8_t* rgb_in = nullptr; uint8_t* rgb_out = nullptr;
    const idc_ref_image* images = nullptr; uint8_t* const* outs = nullptr;
    const int32_t* hint_offsets = nullptr; const idc_hint* hints = nullptr;
    int mode = 0; float mask_value = 0.f, maskcent = 0.f, l_cent = 0.f; unsigned flags = 0;
    float* out_ab = nullptr;
    // has_refs: the batch brings its references, and the network reads the slot's own global inputs (else the handle's, as idc_forward_async)
    bool has_refs = false; idc_batch_refs refs = {};
    // eval (idc_forward_async_eval and later): the score is required, the revealed colours are optional.  taps_call (idc_forward_async_dist):
    // the score is optional too, and a NULL taps is refused; score_call (idc_forward_async_dist_score): then taps may be NULL
    bool eval = false; uint64_t* sse = nullptr; float* hint_colours = nullptr;
    bool taps_call = false; const idc_dist_taps* taps = nullptr;
    bool score_call = false; const idc_dist_score_spec* spec = nullptr; const float* centres = nullptr; const idc_dist_score_out* sout = nullptr;
    // the sample width and the output depth (idc_forward_async_gray; ragged only): gray_bits 0 = [h,w,3] uint8 RGB in `images`, 8 | 16 = one
    // plane [h,w] of uint8 | uint16 in `grays`; out_bits 8 | 16 = [.,.,3] uint8 | uint16 out
    int gray_bits = 0, out_bits = 8; const idc_gray_image* grays = nullptr;
    // the handle's ingest filter as the call was enqueued (idc_set_ingest_filter): IDC_FILTER_BILINEAR leaves every byte of the plan as it was
    int ingest_filter = IDC_FILTER_BILINEAR;
    // painted hint layers (idc_forward_async_layers; ragged only): has_layers = the call brought an idc_batch_layers, whose three parts follow --
    // the table [n] (rgba NULL: that image has no layer), the two parameters of the rule, and where the cell counts go (or nullptr).  Without it
    // every byte of the plan and of the block is as it was.
    bool has_layers = false; const idc_hint_layer* layers = nullptr; int alpha_min = 0, cover = 0; int32_t* cells = nullptr;
    // the handle's output format and matrix as the call was enqueued (idc_set_batch_output): IDC_OUT_RGB leaves every byte of the plan as it was
    int out_format = IDC_OUT_RGB, out_matrix = IDC_YCC_JFIF;
    // the handle's temporal filter as the call was enqueued (idc_set_temporal_filter).  It takes no room in the plan or in the metadata block:
    // on or off, every byte of both is the same
    TemporalParams temporal = temporal_defaults();
    // ... and its motion compensation (idc_set_temporal_motion): no room in either as well
    MotionParams motion = motion_defaults();
    // ... and the hint tracking along its vectors (idc_set_hint_tracking): no room in either as well
    TrackParams track = track_defaults();
};

inline void set_batch_layers(BatchCall& c, const idc_batch_layers* l) {
    c.has_layers = l != nullptr;
    if (l) { c.layers = l->layers; c.alpha_min = l->alpha_min; c.cover = l->cover; c.cells = l->cells; }
}

// image i of a ragged call, whichever table it came in (a plane's samples stand in the place of the bytes)
inline idc_ref_image batch_image(const BatchCall& c, int i) {
    if (c.gray_bits == 0) return c.images[i];
    return {(const uint8_t*)c.grays[i].pix, c.grays[i].h, c.grays[i].w};
}

inline void set_batch_refs(BatchCall& c, const idc_batch_refs* r) {
    c.has_refs = r != nullptr;
    if (r) c.refs = *r;
}

// One host buffer of a call and the bytes of the slot's packed device array it fills (in) or receives (out)
struct Piece { const uint8_t* in; uint8_t* out; size_t in_at, in_bytes, out_at, out_bytes; bool in_pinned, out_pinned; };

struct BatchPlan {
    bool want_rgb = false;               // only an evaluation batch may keep its images on the device
    bool reveal = false, dist = false, score = false, source_out = false;
    int n_hints = 0, kept = 0;           // hints in the caller's list; those that survive clip_hint
    size_t in_bytes = 0, rgb_bytes = 0;  // the packed sources; the packed results that leave the device
    // the metadata block: the kept-hint offsets int[max_batch + 1] at 0, (ragged) the table ImgDesc[max_batch + 1] at table_at, the kept
    // hints HintRect[kept] at hints_at, (reveal) each kept hint's place in the caller's list int[kept] at orig_at
    size_t table_at = 0, hints_at = 0, orig_at = 0, meta_bytes = 0, meta_floor = 0;
    size_t cols_at = 0, cols_bytes = 0;  // the evaluation block: sse uint64[max_batch][3] at 0, then hint_colours float[n_hints][2]
    long long max_tiles = 0, max_pixels = 0;     // joint_tiles / pixels of the largest source
    int bpp_in = 3, bpp_out = 3;         // bytes per pixel of the packed sources (1, 2 or 3) and of the packed source-size results (3 or 6)
    std::vector<Piece> pieces;           // in_pinned / out_pinned: the caller's to fill in (a runtime query); out_pinned without want_rgb: true
    bool ab_pinned = false;              // ... and so is this one, of out_ab
    // antialiased ingestion: naa = the images of the call the pre-pass down-scales (0: the filter is off or no image is larger than the net, and
    // everything above is the whole plan).  Their net-size lattice images [H,W] of bpp_in bytes per pixel lie behind the packed sources in the
    // SAME device array, image k of them at byte aa_at + k * H * W * bpp_in (aa_at is a multiple of 48: a whole number of samples of every
    // format); src_bytes = what that array holds then.  Appended to the metadata block, behind today's: (ragged) the ingestion view
    // ImgDesc[max_batch + 1] at view_at -- the table with every down-scaled image's entry pointing at its net-size image as an H x W source,
    // the others and the closing entry as they are: what the kernels that bring a source to the net size read -- and the pre-pass's
    // ResampleJob[naa] at jobs_at.  aa_tiles = the largest tile count among the jobs.
    int naa = 0, aa_tiles = 0;
    size_t aa_at = 0, src_bytes = 0, view_at = 0, jobs_at = 0;
    // painted hint layers: n_layers = the images of the call that bring one (0: everything above is the whole plan).  The [lh,lw,4] layers lie
    // packed back to back, in image order, in a device array of the slot's OWN (layer_bytes of it; every start is a multiple of 4), one piece
    // each in layer_pieces (in_at = the start; nothing comes back), which travel by copy_runs' rule.  Appended to the metadata block, behind
    // everything above: LayerDesc[max_batch] at layers_at, entry i = {start, lh, lw} or zeros for an image without a layer and past n.
    // layer_blocks = grid.x of the post-pass: the largest layer_blocks (idc_layer.h) among the layers.
    int n_layers = 0, layer_blocks = 0;
    size_t layer_bytes = 0, layers_at = 0;
    std::vector<Piece> layer_pieces;
    bool cells_pinned = false;           // the caller's to fill in, as ab_pinned
    // YCbCr 4:2:0 output (c.out_format != IDC_OUT_RGB and the images leave the device; else ycc_bytes == 0 and everything above is the whole
    // plan): every image's plane block (idc_ycc.h) packed back to back, in image order and without padding, in a device array of the slot's OWN,
    // ycc_bytes of it.  The pieces' out_at / out_bytes then name THAT array: what travels back is the blocks, not the RGB, which stays where the
    // epilogue wrote it (rgb_bytes still sizes it).  Appended to the metadata block, behind everything above: YccDesc[n] at ycc_at.
    // ycc_blocks = grid.x of the post-pass: the largest ycc_blocks among the images.
    size_t ycc_bytes = 0, ycc_at = 0;
    int ycc_blocks = 0;
};

// image i's size as its result has it: the source's own (IDC_BATCH_OUT_SOURCE) or the net's
inline void batch_out_size(const BatchCall& c, int i, int H, int W, int* oh, int* ow) {
    const bool source_out = (c.flags & IDC_BATCH_OUT_SOURCE) != 0;
    *oh = !source_out ? H : c.ragged ? batch_image(c, i).h : c.src_h;
    *ow = !source_out ? W : c.ragged ? batch_image(c, i).w : c.src_w;
}

inline int plan_fail(std::string* err, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (err) *err = buf;
    return code;
}

inline size_t batch_align16(size_t v) { return (v + 15) / 16 * 16; }

// Every check of a call's arguments that needs neither the handle nor the runtime (c.n is in 1..max_batch: the caller checked), then the
// layout.  0, or the status with its text in *err; *p is complete only on 0.
inline int plan_batch(const BatchCall& c, int H, int W, int max_batch, BatchPlan* p, std::string* err) {
    const int n = c.n;
    *p = BatchPlan();
    p->want_rgb = c.ragged ? c.outs != nullptr : c.rgb_out != nullptr;
    p->reveal = c.eval && c.mode == IDC_HINT_REVEAL;
    p->dist = c.eval && c.taps_call;
    p->score = p->dist && c.score_call;
    const bool gray = c.gray_bits != 0;
    if (c.slot < 0 || c.slot > 1) return plan_fail(err, IDC_ERR_INVALID_ARG, "slot %d not in 0..1", c.slot);
    if (gray && c.gray_bits != 8 && c.gray_bits != 16) return plan_fail(err, IDC_ERR_INVALID_ARG, "bits %d is neither 8 nor 16", c.gray_bits);
    if (c.ragged ? (!(gray ? (const void*)c.grays : (const void*)c.images) || !(c.outs || c.eval)) : (!c.rgb_in || !c.rgb_out))
        return plan_fail(err, IDC_ERR_INVALID_ARG, "null image pointer");
    if (c.flags & ~(unsigned)(IDC_BATCH_OUT_SOURCE | (gray ? IDC_BATCH_OUT_RGB16 : 0))) return plan_fail(err, IDC_ERR_INVALID_ARG, "unknown flag bits 0x%x", c.flags);
    if (gray && c.mode == IDC_HINT_REVEAL) return plan_fail(err, IDC_ERR_INVALID_ARG, "IDC_HINT_REVEAL: a greyscale source has no colour to reveal");
    if (c.out_bits == 16 && c.gray_bits != 16) return plan_fail(err, IDC_ERR_INVALID_ARG, "IDC_BATCH_OUT_RGB16 needs 16-bit samples, not %d-bit ones", c.gray_bits);
    if (c.out_bits == 16 && !(c.flags & IDC_BATCH_OUT_SOURCE)) return plan_fail(err, IDC_ERR_INVALID_ARG, "IDC_BATCH_OUT_RGB16 without IDC_BATCH_OUT_SOURCE: the net-size result is 8-bit");
    if (c.out_format != IDC_OUT_RGB && c.out_format != IDC_OUT_I420 && c.out_format != IDC_OUT_NV12)
        return plan_fail(err, IDC_ERR_INVALID_ARG, "output format %d", c.out_format);
    if (c.out_format != IDC_OUT_RGB && c.out_matrix != IDC_YCC_JFIF && c.out_matrix != IDC_YCC_BT709_VIDEO)
        return plan_fail(err, IDC_ERR_INVALID_ARG, "YCbCr matrix %d", c.out_matrix);
    if (c.out_format != IDC_OUT_RGB && c.out_bits == 16)
        return plan_fail(err, IDC_ERR_UNSUPPORTED, "IDC_BATCH_OUT_RGB16 with a YCbCr output format: the planes are 8-bit");
    p->bpp_in = gray ? c.gray_bits / 8 : 3;
    p->bpp_out = c.out_bits == 16 ? 6 : 3;
    size_t full_bytes = 0;               // the packed source-size results
    if (c.mode != IDC_HINT_AB && c.mode != IDC_HINT_RGB && !p->reveal) return plan_fail(err, IDC_ERR_INVALID_ARG, "hint mode %d", c.mode);
    if (c.eval && !c.sse && !p->dist) return plan_fail(err, IDC_ERR_INVALID_ARG, "null sse");
    if (c.eval && c.hint_colours && !p->reveal)
        return plan_fail(err, IDC_ERR_INVALID_ARG, "hint_colours with hint mode %d: only IDC_HINT_REVEAL reveals colours", c.mode);
    if (c.ragged) {
        for (int i = 0; i < n; ++i) {
            const idc_ref_image im = batch_image(c, i);
            if (!im.rgb || (p->want_rgb && !c.outs[i])) return plan_fail(err, IDC_ERR_INVALID_ARG, "image %d: null image pointer", i);
            if (c.gray_bits == 16 && ((uintptr_t)im.rgb & 1)) return plan_fail(err, IDC_ERR_INVALID_ARG, "image %d: 16-bit samples at an odd address", i);
            if (c.out_bits == 16 && p->want_rgb && ((uintptr_t)c.outs[i] & 1)) return plan_fail(err, IDC_ERR_INVALID_ARG, "image %d: 16-bit result at an odd address", i);
            if (im.h < 1 || im.h > 16384 || im.w < 1 || im.w > 16384)
                return plan_fail(err, IDC_ERR_INVALID_ARG, "image %d: source size %dx%d outside 1..16384", i, im.h, im.w);
            p->in_bytes += (size_t)im.h * im.w * p->bpp_in;       // n * 0.8 GB: no overflow in 64 bits
            full_bytes += (size_t)im.h * im.w * p->bpp_out;
        }
        if (p->in_bytes > IDC_BATCH_MAX_SOURCE_BYTES)
            return plan_fail(err, IDC_ERR_INVALID_ARG, "%d sources hold %zu bytes, more than %zu", n, p->in_bytes, (size_t)IDC_BATCH_MAX_SOURCE_BYTES);
        if ((c.flags & IDC_BATCH_OUT_SOURCE) && full_bytes > IDC_BATCH_MAX_SOURCE_BYTES)
            return plan_fail(err, IDC_ERR_INVALID_ARG, "%d source-size results hold %zu bytes, more than %zu", n, full_bytes, (size_t)IDC_BATCH_MAX_SOURCE_BYTES);
    } else {
        if (c.src_h < 1 || c.src_h > 16384 || c.src_w < 1 || c.src_w > 16384)
            return plan_fail(err, IDC_ERR_INVALID_ARG, "source size %dx%d outside 1..16384", c.src_h, c.src_w);
        p->in_bytes = full_bytes = (size_t)n * c.src_h * c.src_w * 3;
        if (p->in_bytes > IDC_BATCH_MAX_SOURCE_BYTES)
            return plan_fail(err, IDC_ERR_INVALID_ARG, "%d sources of %dx%d are more than %zu bytes", n, c.src_h, c.src_w, (size_t)IDC_BATCH_MAX_SOURCE_BYTES);
    }
    if (c.hint_offsets) {
        if (c.hint_offsets[0] != 0) return plan_fail(err, IDC_ERR_INVALID_ARG, "hint_offsets[0] is %d, not 0", c.hint_offsets[0]);
        for (int i = 0; i < n; ++i)
            if (c.hint_offsets[i + 1] < c.hint_offsets[i]) return plan_fail(err, IDC_ERR_INVALID_ARG, "hint_offsets decrease at image %d", i);
        p->n_hints = c.hint_offsets[n];
        if (p->n_hints > IDC_BATCH_MAX_HINTS) return plan_fail(err, IDC_ERR_INVALID_ARG, "%d hints, more than %d", p->n_hints, IDC_BATCH_MAX_HINTS);
        if (p->n_hints > 0 && !c.hints) return plan_fail(err, IDC_ERR_INVALID_ARG, "null hints with a non-zero offset");
    }
    for (int k = 0; k < p->n_hints; ++k) {
        HintRect r;
        if (!clip_hint(c.hints[k], H, W, r)) continue;
        if (c.mode == IDC_HINT_RGB && !(r.c0 >= 0.f && r.c0 <= 255.f && r.c1 >= 0.f && r.c1 <= 255.f && r.c2 >= 0.f && r.c2 <= 255.f))
            return plan_fail(err, IDC_ERR_INVALID_ARG, "hint %d: RGB outside 0..255", k);
        ++p->kept;
    }
    if (c.has_layers) {
        if (!c.ragged) return plan_fail(err, IDC_ERR_INVALID_ARG, "layers with a same-size call");
        if (!c.layers) return plan_fail(err, IDC_ERR_INVALID_ARG, "null layer table");
        if (c.alpha_min < 1 || c.alpha_min > 255) return plan_fail(err, IDC_ERR_INVALID_ARG, "alpha_min %d outside 1..255", c.alpha_min);
        if (c.cover < 0 || c.cover > 255) return plan_fail(err, IDC_ERR_INVALID_ARG, "cover %d outside 0..255", c.cover);
        for (int i = 0; i < n; ++i) {
            const idc_hint_layer& l = c.layers[i];
            if (!l.rgba) continue;
            if (l.h < 1 || l.h > kLayerMaxSide || l.w < 1 || l.w > kLayerMaxSide)
                return plan_fail(err, IDC_ERR_INVALID_ARG, "image %d: layer size %dx%d outside 1..%d", i, l.h, l.w, kLayerMaxSide);
            p->layer_bytes += (size_t)l.h * l.w * 4;              // n * 1 GB: no overflow in 64 bits
            ++p->n_layers;
        }
        if (p->layer_bytes > IDC_BATCH_MAX_SOURCE_BYTES)
            return plan_fail(err, IDC_ERR_INVALID_ARG, "%d layers hold %zu bytes, more than %zu", p->n_layers, p->layer_bytes, (size_t)IDC_BATCH_MAX_SOURCE_BYTES);
        if (p->n_layers > 0 && !(std::isfinite(c.mask_value) && c.mask_value != 0.f))
            return plan_fail(err, IDC_ERR_INVALID_ARG, "a call with a layer needs a finite mask_value != 0");
    }
    const size_t hw = (size_t)H * W, nb = (size_t)max_batch;
    p->source_out = (c.flags & IDC_BATCH_OUT_SOURCE) != 0;
    p->rgb_bytes = p->source_out ? full_bytes : (size_t)n * hw * 3;
    p->table_at = batch_align16((nb + 1) * sizeof(int));
    p->hints_at = c.ragged ? p->table_at + batch_align16((nb + 1) * sizeof(ImgDesc)) : p->table_at;
    p->orig_at = p->hints_at + (size_t)p->kept * sizeof(HintRect);
    p->meta_bytes = p->orig_at + (p->reveal ? (size_t)p->kept * sizeof(int) : 0);
    p->meta_floor = p->hints_at + 256 * (sizeof(HintRect) + sizeof(int));
    p->cols_at = nb * 3 * sizeof(uint64_t);
    p->cols_bytes = c.eval && c.hint_colours ? (size_t)p->n_hints * 2 * sizeof(float) : 0;
    if (c.ragged) {
        size_t at = 0;
        for (int i = 0; i < n; ++i) {
            const idc_ref_image im = batch_image(c, i);
            const size_t px = (size_t)im.h * im.w, sb = px * p->bpp_in, first = at / p->bpp_in;
            p->pieces.push_back({im.rgb, p->want_rgb ? c.outs[i] : nullptr, at, sb, p->source_out ? first * p->bpp_out : (size_t)i * hw * 3,
                                 p->source_out ? px * p->bpp_out : hw * 3, false, false});
            p->max_tiles = p->max_tiles > joint_tiles(im.h, im.w) ? p->max_tiles : joint_tiles(im.h, im.w);
            p->max_pixels = p->max_pixels > (long long)im.h * im.w ? p->max_pixels : (long long)im.h * im.w;
            at += sb;
        }
    } else {
        p->pieces.push_back({c.rgb_in, c.rgb_out, 0, p->in_bytes, 0, p->rgb_bytes, false, false});
        p->max_tiles = joint_tiles(c.src_h, c.src_w);
        p->max_pixels = (long long)c.src_h * c.src_w;
    }
    p->src_bytes = p->in_bytes;
    if (c.ingest_filter == IDC_FILTER_ANTIALIAS) {
        for (int i = 0; i < n; ++i) {
            const int ih = c.ragged ? batch_image(c, i).h : c.src_h, iw = c.ragged ? batch_image(c, i).w : c.src_w;
            if (!resample_applies(ih, iw, H, W)) continue;
            const int tiles = resample_tile_count(W, resample_tile_width(iw, W, gray ? 1 : 3));
            p->aa_tiles = p->aa_tiles > tiles ? p->aa_tiles : tiles;
            ++p->naa;
        }
    }
    if (p->naa > 0) {
        p->aa_at = (p->in_bytes + 47) / 48 * 48;
        p->src_bytes = p->aa_at + (size_t)p->naa * hw * p->bpp_in;
        p->view_at = batch_align16(p->meta_bytes);
        p->jobs_at = c.ragged ? p->view_at + batch_align16((nb + 1) * sizeof(ImgDesc)) : p->view_at;
        p->meta_bytes = p->jobs_at + (size_t)p->naa * sizeof(ResampleJob);
    }
    if (p->n_layers > 0) {
        size_t at = 0;
        for (int i = 0; i < n; ++i) {
            const idc_hint_layer& l = c.layers[i];
            if (!l.rgba) continue;
            const size_t lb = (size_t)l.h * l.w * 4;
            const int blocks = layer_blocks(l.h, l.w, H, W);
            p->layer_pieces.push_back({l.rgba, nullptr, at, lb, 0, 0, false, true});
            p->layer_blocks = p->layer_blocks > blocks ? p->layer_blocks : blocks;
            at += lb;
        }
        p->layers_at = batch_align16(p->meta_bytes);
        p->meta_bytes = p->layers_at + nb * sizeof(LayerDesc);
    }
    if (c.out_format != IDC_OUT_RGB && p->want_rgb) {
        for (int i = 0; i < n; ++i) {
            int oh, ow;
            batch_out_size(c, i, H, W, &oh, &ow);
            const size_t yb = ycc420_bytes(oh, ow);
            if (c.ragged) { p->pieces[i].out_at = p->ycc_bytes; p->pieces[i].out_bytes = yb; }
            p->ycc_bytes += yb;
            p->ycc_blocks = p->ycc_blocks > ycc_blocks(oh, ow) ? p->ycc_blocks : ycc_blocks(oh, ow);
        }
        if (!c.ragged) p->pieces[0].out_bytes = p->ycc_bytes;
        p->ycc_at = batch_align16(p->meta_bytes);
        p->meta_bytes = p->ycc_at + (size_t)n * sizeof(YccDesc);
    }
    return IDC_OK;
}

// The metadata block as the kernels read it, into h_meta (p.meta_bytes of it): offsets of the KEPT hints per image, (ragged) the image table
// with its closing entry, the clipped rectangles, (reveal) their places in the caller's list.
inline void fill_batch_meta(const BatchCall& c, const BatchPlan& p, int H, int W, unsigned char* h_meta) {
    int* m_offs = (int*)h_meta;
    HintRect* m_hints = (HintRect*)(h_meta + p.hints_at);
    int* m_orig = (int*)(h_meta + p.orig_at);
    if (c.ragged) {
        ImgDesc* tab = (ImgDesc*)(h_meta + p.table_at);
        for (int i = 0; i <= c.n; ++i) {           // entry n closes the run: where the next image would begin
            const size_t at = i < c.n ? p.pieces[i].in_at : p.in_bytes;
            tab[i].off = (long long)at; tab[i].first = (long long)(at / p.bpp_in);
            tab[i].h = i < c.n ? batch_image(c, i).h : 0; tab[i].w = i < c.n ? batch_image(c, i).w : 0;
        }
    }
    m_offs[0] = 0;
    for (int i = 0, w = 0; i < c.n; ++i) {
        for (int k = c.hint_offsets ? c.hint_offsets[i] : 0; k < (c.hint_offsets ? c.hint_offsets[i + 1] : 0); ++k) {
            HintRect r;                             // clip_hint fills r even for a hint it drops: only a kept one may reach the block, which has room for `kept`
            if (!clip_hint(c.hints[k], H, W, r)) continue;
            if (p.reveal) m_orig[w] = k;
            m_hints[w++] = r;
        }
        m_offs[i + 1] = w;
    }
    if (p.naa > 0) {                                // the pre-pass's jobs and (ragged) the ingestion view, behind everything above
        const size_t net_bytes = (size_t)H * W * p.bpp_in;
        ResampleJob* jobs = (ResampleJob*)(h_meta + p.jobs_at);
        ImgDesc* view = c.ragged ? (ImgDesc*)(h_meta + p.view_at) : nullptr;
        const ImgDesc* tab = c.ragged ? (const ImgDesc*)(h_meta + p.table_at) : nullptr;
        if (view) view[c.n] = tab[c.n];
        for (int i = 0, k = 0; i < c.n; ++i) {
            const int ih = c.ragged ? tab[i].h : c.src_h, iw = c.ragged ? tab[i].w : c.src_w;
            const size_t at = c.ragged ? (size_t)tab[i].off : (size_t)i * c.src_h * c.src_w * 3;
            if (view) view[i] = tab[i];
            if (!resample_applies(ih, iw, H, W)) continue;
            const size_t dst = p.aa_at + (size_t)k * net_bytes;
            jobs[k++] = resample_job((long long)at, (long long)dst, ih, iw, W, c.gray_bits ? 1 : 3);
            if (view) { view[i].off = (long long)dst; view[i].first = (long long)(dst / p.bpp_in); view[i].h = H; view[i].w = W; }
        }
    }
    if (p.n_layers > 0) {                           // the post-pass's table, behind everything above: the block ends with its max_batch entries
        LayerDesc* tab = (LayerDesc*)(h_meta + p.layers_at);
        const int nb = (int)((p.meta_bytes - p.layers_at) / sizeof(LayerDesc));
        for (int i = 0, k = 0; i < nb; ++i) {
            const bool has = i < c.n && c.layers[i].rgba != nullptr;
            tab[i].off = has ? (long long)p.layer_pieces[k++].in_at : 0;
            tab[i].h = has ? c.layers[i].h : 0; tab[i].w = has ? c.layers[i].w : 0;
        }
    }
    if (p.ycc_bytes > 0) {                          // the output post-pass's table: where each image's RGB lies in the packed results, and its block
        YccDesc* tab = (YccDesc*)(h_meta + p.ycc_at);
        size_t src = 0, dst = 0;
        for (int i = 0; i < c.n; ++i) {
            int oh, ow;
            batch_out_size(c, i, H, W, &oh, &ow);
            tab[i].src = (long long)src; tab[i].dst = (long long)dst; tab[i].h = oh; tab[i].w = ow;
            src += (size_t)oh * ow * 3; dst += ycc420_bytes(oh, ow);
        }
    }
}

// Pieces <-> a packed device array: a pinned buffer travels in place (piece >= 0: between that piece's own buffer and [at, at + bytes) of the
// array), a pageable one through the staging buffer at the piece's own offset (piece < 0: staging and array at the same [at, at + bytes)),
// and neighbouring staged pieces go as ONE copy.
struct CopyOp { int piece; size_t at, bytes; };

inline std::vector<CopyOp> copy_runs(const std::vector<Piece>& pieces, bool to_device) {
    std::vector<CopyOp> ops;
    size_t run0 = 0, run1 = 0;                      // staged bytes [run0, run1) not yet issued
    auto flush = [&]() {
        if (run1 != run0) ops.push_back({-1, run0, run1 - run0});
        run0 = run1;
    };
    for (int i = 0; i < (int)pieces.size(); ++i) {
        const Piece& p = pieces[i];
        const size_t at = to_device ? p.in_at : p.out_at, bytes = to_device ? p.in_bytes : p.out_bytes;
        const bool pinned = to_device ? p.in_pinned : p.out_pinned;
        if (!pinned && at == run1) { run1 = at + bytes; continue; }
        flush();
        if (!pinned) { run0 = at; run1 = at + bytes; continue; }
        ops.push_back({i, at, bytes});
        run0 = run1 = at + bytes;
    }
    flush();
    return ops;
}

}  // namespace idc

#endif  // IDC_BATCH_H
