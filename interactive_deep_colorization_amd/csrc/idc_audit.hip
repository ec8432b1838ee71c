// idc_audit.hip -- range audit of a layer's STORED output (idc_set_range_audit): one streaming reduction over the tensor as the next layer will
// read it, for every storage form the engine uses -- fp32 NHWC, one bf16 / fp16 plane, or the 2 / 3 planes of the operand-split precisions (value =
// sum of the parts in fp32, hi first: the order split_to_nchw_kernel uses, so idc_get_activation shows the same numbers).  Padding channels
// (CoutPad beyond cout) are skipped.  Bandwidth-bound: 16-byte loads, four in flight per lane, a wave reduction by __shfl_xor, one LDS step per
// workgroup, then at most four vector atomics per workgroup into the layer's 32-byte record.
#include <hip/hip_runtime.h>

#include "idc_kernels.h"

namespace idc {

namespace {

struct AuditAcc {
    float mx = 0.f;
    unsigned sat = 0, tiny = 0, bad = 0;       // per lane: a lane sees < 2^32 values of any tensor the engine can hold
};

template <bool SAT>
__device__ __forceinline__ void audit_value(float v, AuditAcc& r) {
    const float av = fabsf(v);
    if (!(av < INFINITY)) { ++r.bad; return; }                 // NaN / inf: counted, kept out of max_abs
    r.mx = fmaxf(r.mx, av);
    if (SAT && av >= 65504.f) ++r.sat;
    if (av != 0.f && av < 6.103515625e-05f) ++r.tiny;          // 2^-14: fp16's smallest normal
}

__device__ __forceinline__ float half_bits_to_f32(unsigned short q, bool f16) {
    return f16 ? (float)__builtin_bit_cast(_Float16, q) : __uint_as_float((unsigned)q << 16);
}

// FORM 0: fp32 [pixel][Cpad], 4 channels per 16-byte load.  FORM 1: 16-bit parts [pixel][parts][Cpad], 8 channels per load per part.
template <int FORM>
__device__ __forceinline__ void audit_vec(const void* __restrict__ src, long long vec, int vpp, int C, int Cpad, int parts, bool f16, AuditAcc& r) {
    const long long pix = vec / vpp;
    const int cv = (int)(vec - pix * vpp);
    if constexpr (FORM == 0) {
        const int c0 = cv * 4;
        if (c0 >= C) return;
        const float4 q = *(const float4*)((const float*)src + pix * Cpad + c0);
        const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) if (c0 + j < C) audit_value<false>(v[j], r);
    } else {
        const int c0 = cv * 8;
        if (c0 >= C) return;
        const unsigned short* const p = (const unsigned short*)src + (pix * parts) * Cpad + c0;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int pt = 0; pt < parts; ++pt) {
            const uint4 q = *(const uint4*)(p + (long long)pt * Cpad);
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[2 * j] += half_bits_to_f32((unsigned short)(w[j] & 0xffffu), f16);
                v[2 * j + 1] += half_bits_to_f32((unsigned short)(w[j] >> 16), f16);
            }
        }
        if (f16) {
#pragma unroll
            for (int j = 0; j < 8; ++j) if (c0 + j < C) audit_value<true>(v[j], r);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) if (c0 + j < C) audit_value<false>(v[j], r);
        }
    }
}

template <int FORM>
__global__ __launch_bounds__(256) void range_audit_kernel(const void* __restrict__ src, long long nvec, int vpp, int C, int Cpad, int parts, int f16,
                                                          AuditRecord* __restrict__ rec) {
    AuditAcc r;
    const long long stride = (long long)gridDim.x * 256;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {           // four independent 16-byte loads (x parts) in flight per lane
#pragma unroll
        for (int u = 0; u < 4; ++u) audit_vec<FORM>(src, i + u * stride, vpp, C, Cpad, parts, f16 != 0, r);
    }
    for (; i < nvec; i += stride) audit_vec<FORM>(src, i, vpp, C, Cpad, parts, f16 != 0, r);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        r.mx = fmaxf(r.mx, __shfl_xor(r.mx, d));
        r.sat += __shfl_xor(r.sat, d); r.tiny += __shfl_xor(r.tiny, d); r.bad += __shfl_xor(r.bad, d);
    }
    __shared__ float s_mx[4];
    __shared__ unsigned s_cnt[4][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mx[wave] = r.mx; s_cnt[wave][0] = r.sat; s_cnt[wave][1] = r.tiny; s_cnt[wave][2] = r.bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float mx = s_mx[0];
        unsigned long long cnt[3] = {s_cnt[0][0], s_cnt[0][1], s_cnt[0][2]};
        for (int w = 1; w < 4; ++w) { mx = fmaxf(mx, s_mx[w]); for (int k = 0; k < 3; ++k) cnt[k] += s_cnt[w][k]; }
        if (mx > 0.f) atomicMax(&rec->max_abs_bits, __float_as_uint(mx));      // non-negative floats order like their bit patterns
        if (cnt[0]) atomicAdd(&rec->n_saturated, cnt[0]);
        if (cnt[1]) atomicAdd(&rec->n_tiny, cnt[1]);
        if (cnt[2]) atomicAdd(&rec->n_nonfinite, cnt[2]);
    }
}

}  // namespace

hipError_t launch_range_audit(const void* src, long long npix, int C, int Cpad, int parts, int f16, AuditRecord* rec, hipStream_t s) {
    if (!src || !rec || npix <= 0 || C <= 0 || Cpad < C || Cpad % 8 != 0 || parts < 0 || parts > 3) return hipErrorInvalidValue;
    const int vpp = parts == 0 ? Cpad / 4 : Cpad / 8;          // 16-byte vectors per pixel (per part)
    const long long nvec = npix * vpp;
    const int blocks = grid_blocks(GridTag::range_audit, (nvec + 256 * 4 - 1) / (256 * 4), 2048);      // 256 CUs x 8 workgroups, grid-stride beyond
    if (parts == 0) hipLaunchKernelGGL(range_audit_kernel<0>, dim3(blocks), dim3(256), 0, s, src, nvec, vpp, C, Cpad, parts, f16, rec);
    else hipLaunchKernelGGL(range_audit_kernel<1>, dim3(blocks), dim3(256), 0, s, src, nvec, vpp, C, Cpad, parts, f16, rec);
    return hipGetLastError();
}

}  // namespace idc
