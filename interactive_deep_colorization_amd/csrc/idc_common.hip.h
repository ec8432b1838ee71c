// idc_common.hip.h -- the one device header of the conv kernel families: vector typedefs, the tuning harness's cycle stamps, MFMA wrappers on 16-byte
// fragments, 16-bit packing, the XCD-aware block remap, the small-tile epilogue, and what the 16x16x32 throughput kernels share -- the accumulator set
// f32x4 acc[4][8] (bias after the K loop, the (BN, ReLU) pack of one site), the wave-private transpose tile (tile_write16 / tile_read_lines /
// tile_store_lines) and the operand-split epilogue.
#pragma once
#include <type_traits>

#include "idc_kernels.h"
#include "idc_layout.h"

namespace idc {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // 16-byte slot held in registers
typedef __attribute__((ext_vector_type(16))) float f32x16;    // one 32x32 MFMA accumulator tile

// in-kernel cycle stamps for the tuning harness (tools/ablate): compiled out of the library
#ifdef IDC_TIMING
extern __device__ long long* g_idc_dbg;      // defined in idc_igemm.hip
#define IDC_STAMP(i) do { if (tid == 0) g_idc_dbg[(size_t)blockIdx.x * 16 + (i)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define IDC_STAMP(i) do {} while (0)
#endif
#ifdef IDC_TIMING_FINE
#define IDC_STAMP_FINE(i) IDC_STAMP(i)
#else
#define IDC_STAMP_FINE(i) do {} while (0)
#endif

// ------------------------------------------------------------------------------------------------
// MFMA wrappers on 16-byte fragments.  A lane (row/col = lane&15, group g = lane>>4) holds the
// 16-byte slot (ks*4+g) of its row; the K index it stands for is the same permutation for both
// operands, so the contraction is exact whatever the order.
// ------------------------------------------------------------------------------------------------
template <typename T> struct Mma;
template <> struct Mma<__bf16> {
    static __device__ __forceinline__ void run(f32x4& acc, const u32x4& w, const u32x4& x) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w),
                                                      __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static __device__ __forceinline__ void run(f32x4& acc, const u32x4& w, const u32x4& x) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(w.x), __uint_as_float(x.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(w.y), __uint_as_float(x.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(w.z), __uint_as_float(x.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(w.w), __uint_as_float(x.w), acc, 0, 0, 0);
    }
};

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    // one v_cvt_pk_bf16_f32 (RNE) as a VECTOR conversion: from `(__bf16)lo | (__bf16)hi << 16` the vectoriser pairs the conversions of NEIGHBOURING packs
    // and un-shuffles them with and / shift / two SDWA ors -- six instructions for two dwords instead of two (round 5: the epilogues are VALU-bound).
    // (Not inline asm: the hazard recogniser does not see an asm's reads of MFMA results, and the scheduler may move it next to the MFMAs.)
    typedef float f32x2_pk __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_pk __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_pk){lo, hi}, bf16x2_pk));
}

// IDC_FP16X3: two fp16 values (RNE) in one dword; inputs are clamped to the fp16 range first (a value beyond +-65504 saturates instead of becoming inf)
__device__ __forceinline__ unsigned pack_f16x2(float lo, float hi) {
    typedef float f32x2_pk __attribute__((ext_vector_type(2)));
    typedef _Float16 f16x2_pk __attribute__((ext_vector_type(2)));
    const float a = __builtin_fminf(__builtin_fmaxf(lo, -65504.f), 65504.f), b = __builtin_fminf(__builtin_fmaxf(hi, -65504.f), 65504.f);
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_pk){a, b}, f16x2_pk));
}
// two fp32 -> one dword of 16-bit values: bf16 (RNE) or fp16 (RNE, clamped)
template <bool F16> __device__ __forceinline__ unsigned pack16x2(float lo, float hi) {
    if constexpr (F16) return pack_f16x2(lo, hi); else return pack_bf16x2(lo, hi);
}
__device__ __forceinline__ float f16_lo_to_f32(unsigned q) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(q & 0xffffu)); }
__device__ __forceinline__ float f16_hi_to_f32(unsigned q) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(q >> 16)); }

// One 16x16x32 MFMA step on two 16-byte fragments: bf16 (every precision but IDC_FP16X3 / IDC_FP16) or fp16 operands, fp32 accumulate.
template <bool F16>
__device__ __forceinline__ f32x4 mma_16x16x32(const u32x4& a, const u32x4& b, const f32x4& c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// XCD-aware, bijective block remap: hardware places block b on XCD b%8; give each XCD a
// contiguous range of the logical order so neighbouring tiles (same weights, shared halo) share
// one L2.  Speed only -- any placement is correct.
__device__ __forceinline__ int xcd_remap(int b, int nb) {
    const int xcd = b & 7, q = nb >> 3, r = nb & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (b >> 3);
}


// Fused epilogue arithmetic for 16 consecutive output channels of one pixel (in place):
// v = act(v + bias [+ resid]) [* bn_scale + bn_shift]
__device__ __forceinline__ void epilogue_values16(const ConvArgs& a, float (&v)[16], size_t oidx, const float* bias,
                                                  const float* bsc, const float* bsh, bool has_bn,
                                                  const float* ishift = nullptr) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] += bias[i];
    if (a.resid != nullptr) {
        if (a.resid_bf16) {
            const uint4* rp = (const uint4*)((const unsigned short*)a.resid + oidx);
            const uint4 r0 = rp[0], r1 = rp[1];
            const unsigned rr[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                v[2 * q] += __uint_as_float(rr[q] << 16);
                v[2 * q + 1] += __uint_as_float(rr[q] & 0xffff0000u);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 rv = *(const float4*)((const float*)a.resid + oidx + q * 4);
                v[q * 4 + 0] += rv.x; v[q * 4 + 1] += rv.y; v[q * 4 + 2] += rv.z; v[q * 4 + 3] += rv.w;
            }
        }
    }
    if (a.act == 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = fmaxf(v[i], 0.f);
    } else if (a.act == 2) {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = v[i] > 0.f ? v[i] : 0.2f * v[i];
    }
    if (has_bn) {
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = fmaf(v[i], bsc[i], bsh[i]);
    }
    if (ishift != nullptr) {                     // per-image vector (16 consecutive channels) after the BN affine
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 g = *(const float4*)(ishift + q * 4);
            v[q * 4 + 0] += g.x; v[q * 4 + 1] += g.y; v[q * 4 + 2] += g.z; v[q * 4 + 3] += g.w;
        }
    }
}

__device__ __forceinline__ void pack16_bf16(const float (&v)[16], uint4& p0, uint4& p1) {
    p0.x = pack_bf16x2(v[0], v[1]);   p0.y = pack_bf16x2(v[2], v[3]);
    p0.z = pack_bf16x2(v[4], v[5]);   p0.w = pack_bf16x2(v[6], v[7]);
    p1.x = pack_bf16x2(v[8], v[9]);   p1.y = pack_bf16x2(v[10], v[11]);
    p1.z = pack_bf16x2(v[12], v[13]); p1.w = pack_bf16x2(v[14], v[15]);
}

// epilogue_values16 + a direct store from the MFMA layout: 32 B (bf16) or 64 B (fp32) per lane.
template <bool OUT_BF16>
__device__ __forceinline__ void epilogue16(const ConvArgs& a, float (&v)[16], size_t oidx, const float* bias,
                                           const float* bsc, const float* bsh, bool has_bn,
                                           const float* ishift = nullptr) {
    epilogue_values16(a, v, oidx, bias, bsc, bsh, has_bn, ishift);
    if (!OUT_BF16 && a.out_parts > 0) {
        // fp32 island of an operand-split handle (conv1_1): the result enters the split stack as out_parts bf16 planes per pixel,
        // hi = rne(v), next = rne(v - hi), ... (each remainder exact in fp32); a pixel of the split tensor is [part][CoutPad]
        const int CoutPad = a.ncg * kCoutGroup, np = a.out_parts;
        const size_t co0 = oidx % (size_t)CoutPad;
        unsigned short* o = (unsigned short*)a.out + (oidx - co0) * np + co0;
        for (int p = 0; p < np; ++p) {
            uint4 p0, p1;
            if (a.split_f16) {                                 // IDC_FP16X3: fp16 parts (values clamped to the fp16 range first)
                unsigned w[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const _Float16 h0 = (_Float16)fminf(fmaxf(v[2 * e], -65504.f), 65504.f), h1 = (_Float16)fminf(fmaxf(v[2 * e + 1], -65504.f), 65504.f);
                    w[e] = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
                    v[2 * e] -= (float)h0; v[2 * e + 1] -= (float)h1;
                }
                *(uint4*)(o + (size_t)p * CoutPad) = uint4{w[0], w[1], w[2], w[3]};
                *(uint4*)(o + (size_t)p * CoutPad + 8) = uint4{w[4], w[5], w[6], w[7]};
                continue;
            }
            pack16_bf16(v, p0, p1);
            *(uint4*)(o + (size_t)p * CoutPad) = p0;
            *(uint4*)(o + (size_t)p * CoutPad + 8) = p1;
            const unsigned w[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[2 * e] -= __uint_as_float(w[e] << 16); v[2 * e + 1] -= __uint_as_float(w[e] & 0xffff0000u); }
        }
    } else if (!OUT_BF16 || a.out_f32) {
        float* o = (float*)a.out + oidx;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(float4*)(o + q * 4) = float4{v[q * 4 + 0], v[q * 4 + 1], v[q * 4 + 2], v[q * 4 + 3]};
    } else {
        unsigned short* o = (unsigned short*)a.out + oidx;
        uint4 p0, p1;
        pack16_bf16(v, p0, p1);
        *(uint4*)(o) = p0;
        *(uint4*)(o + 8) = p1;
    }
}

__device__ __forceinline__ void load16(float (&dst)[16], const float* src) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = *(const float4*)(src + q * 4);
        dst[q * 4 + 0] = v.x; dst[q * 4 + 1] = v.y; dst[q * 4 + 2] = v.z; dst[q * 4 + 3] = v.w;
    }
}


template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ------------------------------------------------------------------------------------------------
// The wave-private transpose tile of the throughput kernels: [32 sites][64 couts] of 16-bit values, 128-byte rows, 16-byte slot ^ (site & 7).
// A lane writes its 16 consecutive couts of one site (slots s0, s0 + 1), the wave reads the tile back as lane = (site rr = lane >> 3 of each
// group of 8, 8 couts cc = lane & 7), so that every global store covers whole 128-byte lines.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_write16(char* tb16, int site, int s0, const unsigned (&pk)[8]) {
    *(uint4*)(tb16 + site * 128 + ((s0 ^ (site & 7)) * 16)) = uint4{pk[0], pk[1], pk[2], pk[3]};
    *(uint4*)(tb16 + site * 128 + (((s0 + 1) ^ (site & 7)) * 16)) = uint4{pk[4], pk[5], pk[6], pk[7]};
}
// THE RULE: all four lines of the tile are read, and the reads retired, before the first store's bounds check -- written as read / check / store per line
// the compiler sinks each LDS read under its store's bounds check (read - wait - store, four times in a row): 2.6 k cycles per pixel row, 2 % of the
// N = 32 forward (profiles/r05_epilogue.txt, profiles/r05_v2p_tap_stamps.txt).  o[i] = line i (site i*8 + rr) of the tile.
__device__ __forceinline__ void tile_read_lines(const char* tb16, int rr, int cc, uint4 (&o)[4]) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // same-wave LDS ops are in order: the tile is complete
    auto line = [&](int i) { const int row = i * 8 + rr; return *(const uint4*)(tb16 + row * 128 + ((cc ^ (row & 7)) * 16)); };
    o[0] = line(0); o[1] = line(1); o[2] = line(2); o[3] = line(3);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // reads retired: the tile is free for the next row
}
// ... and put(i, line) for the four lines, with the caller's own addressing and bounds check.  (A put that computes a 64-bit element index per line --
// conv_igemm_v2m, split_epilogue -- is built AFTER tile_read_lines instead: built before the waits, the same source compiles to another schedule of that
// arithmetic; profiles/shared_epilogue.txt.)
template <typename Put>
__device__ __forceinline__ void tile_store_lines(const char* tb16, int rr, int cc, Put&& put) {
    uint4 o[4];
    tile_read_lines(tb16, rr, cc, o);
    put(0, o[0]); put(1, o[1]); put(2, o[2]); put(3, o[3]);
}

// ------------------------------------------------------------------------------------------------
// The accumulator set of the 16x16x32 throughput kernels (conv_igemm_v2m / v2p, conv_ds_fused_m and their split forms): f32x4 acc[4][8], lane
// (site r16 = lane & 15, group g16 = lane >> 4) register j of acc[mi][pt] is cout g16*16 + mi*4 + j of the wave's 64 at site (pixel row pt >> 1,
// column (pt & 1)*16 + r16).  bp addresses the lane's first cout (wave's cout base + g16*16).
// ------------------------------------------------------------------------------------------------
// acc = acc * sc + bias: sc = *acc_scale (2^-s of weights packed as w * 2^s, IDC_FP16X3) or 1 -- fma(x, 1, b) is x + b rounded once, the bf16 parts' sum
__device__ __forceinline__ void add_bias_after_k(const float* bp, f32x4 (&acc)[4][8], const float* acc_scale = nullptr) {
    const float sc = acc_scale != nullptr ? *acc_scale : 1.f;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const float4 bq = *(const float4*)(bp + mi * 4);
#pragma unroll
        for (int pt = 0; pt < 8; ++pt) {
            acc[mi][pt][0] = fmaf(acc[mi][pt][0], sc, bq.x); acc[mi][pt][1] = fmaf(acc[mi][pt][1], sc, bq.y);
            acc[mi][pt][2] = fmaf(acc[mi][pt][2], sc, bq.z); acc[mi][pt][3] = fmaf(acc[mi][pt][3], sc, bq.w);
        }
    }
}
// the 16 couts of site pt as eight dwords of 16-bit values: ReLU, BN affine, round.  (BN, RELU) are COMPILE-TIME: as run-time `if`s inside the unrolled
// element loops the compiler keeps a uniform branch per packed pair (tools/check_kernel_shape.py holds the kernels to a branch budget).
template <bool F16, bool BN, bool RELU>
__device__ __forceinline__ void pack_site16(const f32x4 (&acc)[4][8], int pt, const f32x4 (&bsc)[4], const f32x4 (&bsh)[4], unsigned (&pk)[8]) {
    typedef short s16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float v0 = acc[mi][pt][2 * e], v1 = acc[mi][pt][2 * e + 1];
            if constexpr (BN) {
                if constexpr (RELU) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
                pk[mi * 2 + e] = pack16x2<F16>(fmaf(v0, bsc[mi][2 * e], bsh[mi][2 * e]), fmaf(v1, bsc[mi][2 * e + 1], bsh[mi][2 * e + 1]));
            } else {
                unsigned p = pack16x2<F16>(v0, v1);
                if constexpr (RELU) p = __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, p), s16x2{0, 0}));
                pk[mi * 2 + e] = p;
            }
        }
}

// Epilogue of the operand-split kernels: lane (site r16, group g16) holds couts g16*16 + mi*4 + j of its wave's 64 at site (pixel row pt >> 1,
// column (pt & 1)*16 + r16) in acc[mi][pt][j].  value = BN(act(acc + fp32 shortcut sum)) + per-image shift, all fp32; then either an fp32 NHWC store
// straight from the MFMA layout (out_parts = 0) or out_parts bf16 planes hi = rne(v), next = rne(v - hi), ... (each remainder is exact in fp32), every
// plane through the wave-private [32 sites][64 couts] bf16 transpose tile so that stores cover whole 128-byte lines.
template <int WCO, bool F16 = false>
__device__ __forceinline__ void split_epilogue(const ConvArgs& a, f32x4 (&acc)[4][8], char* smem, int n, int ty0, int tx0, int wpx, int cow, int ro, int cof) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g16 = lane >> 4;
    const int Hs = a.Hs, Ws = a.Ws, so = a.so, Wout = Ws * so, Hout = Hs * so;
    const int CoutPad = a.ncg * kCoutGroup;
    const int np = a.out_parts;
    const float* const resid = (const float*)a.resid;
    const bool has_bn = a.bn_scale != nullptr, has_shift = a.img_shift != nullptr;
    f32x4 bsc[4], bsh[4], ish[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        bsc[mi] = f32x4{1.f, 1.f, 1.f, 1.f}; bsh[mi] = f32x4{0.f, 0.f, 0.f, 0.f}; ish[mi] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (has_bn) {
            const float4 s4 = *(const float4*)(a.bn_scale + cow + g16 * 16 + mi * 4);
            const float4 t4 = *(const float4*)(a.bn_shift + cow + g16 * 16 + mi * 4);
            bsc[mi] = f32x4{s4.x, s4.y, s4.z, s4.w}; bsh[mi] = f32x4{t4.x, t4.y, t4.z, t4.w};
        }
        if (has_shift) {
            const float4 u4 = *(const float4*)(a.img_shift + (size_t)n * CoutPad + cow + g16 * 16 + mi * 4);
            ish[mi] = f32x4{u4.x, u4.y, u4.z, u4.w};
        }
    }
    char* const tb16 = smem + wave * 4096;
    const int rr = lane >> 3, cc = lane & 7;
    const int co8 = cow + cc * 8;
    auto rows = [&](auto act_c) __attribute__((always_inline)) {
        constexpr int ACT = decltype(act_c)::value;
#pragma unroll
        for (int pj = 0; pj < 4; ++pj) {
            const int sy = ty0 + wpx * 4 + pj;
            f32x4 v[2][4];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int pt = pj * 2 + hf, sx = tx0 + hf * 16 + r16;
                const bool inb = sy < Hs && sx < Ws;
                const size_t opix = ((size_t)n * Hout + (sy * so + ro)) * Wout + (sx * so + cof);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    f32x4 x = acc[mi][pt];
                    if (resid != nullptr && inb) {
                        const float4 q = *(const float4*)(resid + opix * CoutPad + cow + g16 * 16 + mi * 4);
                        x += f32x4{q.x, q.y, q.z, q.w};
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float e = x[j];
                        if constexpr (ACT == 1) e = fmaxf(e, 0.f);
                        else if constexpr (ACT == 2) e = fmaxf(e, 0.2f * e);
                        x[j] = fmaf(e, bsc[mi][j], bsh[mi][j]) + ish[mi][j];
                    }
                    v[hf][mi] = x;
                }
                if (np == 0 && inb) {
                    float* const op = (float*)a.out + opix * CoutPad + cow + g16 * 16;
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) *(float4*)(op + mi * 4) = float4{v[hf][mi][0], v[hf][mi][1], v[hf][mi][2], v[hf][mi][3]};
                }
            }
            for (int p = 0; p < np; ++p) {
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int site = hf * 16 + r16;
                    unsigned pk[8];
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            if constexpr (F16) {
                                const unsigned q = pack_f16x2(v[hf][mi][2 * e], v[hf][mi][2 * e + 1]);
                                pk[mi * 2 + e] = q;
                                v[hf][mi][2 * e] -= f16_lo_to_f32(q);                      // exact, as below (11-bit parts)
                                v[hf][mi][2 * e + 1] -= f16_hi_to_f32(q);
                            } else {
                            const unsigned q = pack_bf16x2(v[hf][mi][2 * e], v[hf][mi][2 * e + 1]);
                            pk[mi * 2 + e] = q;
                            v[hf][mi][2 * e] -= __uint_as_float(q << 16);              // exact: the remainder of a round-to-nearest fits fp32
                            v[hf][mi][2 * e + 1] -= __uint_as_float(q & 0xffff0000u);
                            }
                        }
                    tile_write16(tb16, site, g16 * 2, pk);
                }
                uint4 o[4];
                tile_read_lines(tb16, rr, cc, o);
                auto put = [&](int i, const uint4& o) {
                    const int sx = tx0 + i * 8 + rr;
                    if (sy < Hs && sx < Ws) {
                        const size_t oidx = ((((size_t)n * Hout + (sy * so + ro)) * Wout + (sx * so + cof)) * np + p) * CoutPad + co8;
                        *(uint4*)((unsigned short*)a.out + oidx) = o;
                    }
                };
                put(0, o[0]); put(1, o[1]); put(2, o[2]); put(3, o[3]);
            }
        }
    };
    if (a.act == 1) rows(std::integral_constant<int, 1>{});
    else if (a.act == 2) rows(std::integral_constant<int, 2>{});
    else rows(std::integral_constant<int, 0>{});
}

}  // namespace idc
