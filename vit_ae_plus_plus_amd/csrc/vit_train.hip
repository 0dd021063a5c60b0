// Backward of the parts of the encoder-only model that the masked autoencoder does not have (HBM bound):
//   * sequence assembly with a TRAINABLE position table: x = cat(cls_token, tok) + pos_embed (reference model/vit.py:269-272)
//   * the token reduction in front of the classifier: global average pool over the patch tokens, or the cls row
//     (reference model/vit.py:277-282).
// The kernels move one or two float4 per lane and instruction; sums run over the batch in a fixed order inside one thread, so the
// results are bitwise reproducible (no atomics).
#include "common.hpp"
#include "vitae_hip.h"

namespace {

// One thread owns four columns of one token row n in [0, L]: it walks the batch, copies dx[b, n] to dtok[b, n - 1] (n >= 1)
// and keeps the running sum for dpos[n] (and dcls when n == 0).  Four samples' loads are in flight at a time; the additions
// stay in sample order.
__global__ __launch_bounds__(256) void vit_assemble_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dtok,
                                                               __bf16* __restrict__ dtok16, float* __restrict__ dpos,
                                                               float* __restrict__ dcls, int B, int L, int D4, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)(L + 1) * D4) return;
    const int n = (int)(i / D4), c = (int)(i - (long)n * D4);
    const long bstride = (long)(L + 1) * D4;      // in float4 units
    const f32x4* src = reinterpret_cast<const f32x4*>(dx) + (long)n * D4 + c;
    f32x4* out = (dtok && n > 0) ? reinterpret_cast<f32x4*>(dtok) + (long)(n - 1) * D4 + c : nullptr;
    bf16x4* out16 = (dtok16 && n > 0) ? reinterpret_cast<bf16x4*>(dtok16) + (long)(n - 1) * D4 + c : nullptr;
    const long ostride = (long)L * D4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    auto emit = [&](int b, const f32x4& v) {
        if (out) out[(long)b * ostride] = v;
        if (out16) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
            out16[(long)b * ostride] = o;
        }
        s += v;
    };
    int b = 0;
    for (; b + 4 <= B; b += 4) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = src[(long)(b + u) * bstride];
#pragma unroll
        for (int u = 0; u < 4; ++u) emit(b + u, v[u]);
    }
    for (; b < B; ++b) emit(b, src[(long)b * bstride]);
    if (dpos) {
        f32x4* p = reinterpret_cast<f32x4*>(dpos) + (long)n * D4 + c;
        *p = accumulate ? *p + s : s;
    }
    if (dcls && n == 0) {
        f32x4* p = reinterpret_cast<f32x4*>(dcls) + c;
        *p = accumulate ? *p + s : s;
    }
}

// dx[b, n] = mode 1 (global pool): n >= 1 ? dsel[b] / (N - 1) : 0;  mode 0 (cls row): n == 0 ? dsel[b] : 0.
// One float4 of dx per thread; every element of dx is written.
__global__ __launch_bounds__(256) void token_select_bwd_kernel(const float* __restrict__ dsel, float* __restrict__ dx, int N, int D4,
                                                               int mode, float denom) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= (long)N * D4) return;
    const int n = (int)(i / D4), c = (int)(i - (long)n * D4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (mode ? n > 0 : n == 0) v = reinterpret_cast<const f32x4*>(dsel)[(long)b * D4 + c] / denom;
    reinterpret_cast<f32x4*>(dx)[(long)b * N * D4 + i] = v;
}

// The same dx plus what the bf16 backward chain needs on entry, in ONE launch: dx16 [Mpad, D] = bf16(dx) with rows B N .. Mpad - 1
// written as zero (the weight-gradient GEMMs reduce over Mpad rows), and colsum[c] = sum of column c of dx (the fc2 bias gradient of
// the top block).  One thread owns eight columns of one row: two float4 stores of dx, one 16-byte store of dx16.  The threads of
// row 0 also own colsum for their columns: every token row of a sample holds the same value v_b (or zero), so its column sum is
// (N - 1) v_b (mode 1, one rounding) or v_b (mode 0), and the samples are added in order b = 0, 1, ..: no atomics, the same bits
// on every call.
__global__ __launch_bounds__(256) void token_select_bwd16_kernel(const float* __restrict__ dsel, float* __restrict__ dx,
                                                                 __bf16* __restrict__ dx16, float* __restrict__ colsum, int B, int N,
                                                                 int Mpad, int D8, int mode, float denom) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Mpad * D8) return;
    const int row = (int)(i / D8), c = (int)(i - (long)row * D8);
    const int M = B * N;
    const f32x4* sel = reinterpret_cast<const f32x4*>(dsel) + 2 * c;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    if (row < M) {
        const int b = row / N, n = row - b * N;
        if (mode ? n > 0 : n == 0) {
            lo = sel[(long)b * 2 * D8] / denom;
            hi = sel[(long)b * 2 * D8 + 1] / denom;
        }
        f32x4* out = reinterpret_cast<f32x4*>(dx) + i * 2;
        out[0] = lo;
        out[1] = hi;
    }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = (__bf16)lo[e]; o[4 + e] = (__bf16)hi[e]; }
    reinterpret_cast<bf16x8*>(dx16)[i] = o;
    if (row == 0 && colsum) {
        const float rows = mode ? (float)(N - 1) : 1.0f;
        f32x4 slo = {0.f, 0.f, 0.f, 0.f}, shi = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < B; ++b) {
            slo += (sel[(long)b * 2 * D8] / denom) * rows;
            shi += (sel[(long)b * 2 * D8 + 1] / denom) * rows;
        }
        f32x4* cs = reinterpret_cast<f32x4*>(colsum) + 2 * c;
        cs[0] = slo;
        cs[1] = shi;
    }
}

}  // namespace

extern "C" int vitae_vit_assemble_bwd(const float* dx, float* dtok, void* dtok_bf16, float* dpos, float* dcls, int B, int L,
                                      int D, int accumulate, void* stream) {
    if (!dx || (!dtok && !dtok_bf16 && !dpos && !dcls) || B <= 0 || L <= 0 || D <= 0) return VITAE_ERR_INVALID_ARG;
    if ((((uintptr_t)dx | (uintptr_t)dtok | (uintptr_t)dpos | (uintptr_t)dcls) & 15) || ((uintptr_t)dtok_bf16 & 7))
        return VITAE_ERR_INVALID_ARG;
    if (D & 3) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const int D4 = D / 4;
    hipLaunchKernelGGL(vit_assemble_bwd_kernel, dim3(cdiv((long)(L + 1) * D4, 256)), dim3(256), 0, (hipStream_t)stream, dx, dtok,
                       reinterpret_cast<__bf16*>(dtok_bf16), dpos, dcls, B, L, D4, accumulate);
    return vitae_launch_status();
}

extern "C" int vitae_token_select_bwd(const float* dsel, float* dx, int B, int N, int D, int mode, void* stream) {
    if (!dsel || !dx || B <= 0 || N <= 0 || D <= 0 || (mode != 0 && mode != 1) || (mode == 1 && N < 2)) return VITAE_ERR_INVALID_ARG;
    if (((uintptr_t)dsel | (uintptr_t)dx) & 15) return VITAE_ERR_INVALID_ARG;
    if ((D & 3) || B > 65535) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const int D4 = D / 4;
    hipLaunchKernelGGL(token_select_bwd_kernel, dim3(cdiv((long)N * D4, 256), B), dim3(256), 0, (hipStream_t)stream, dsel, dx, N, D4,
                       mode, mode ? (float)(N - 1) : 1.0f);
    return vitae_launch_status();
}

extern "C" int vitae_token_select_bwd16(const float* dsel, float* dx, void* dx_bf16, float* colsum, int B, int N, int Mpad, int D,
                                        int mode, void* stream) {
    if (!dsel || !dx || !dx_bf16 || B <= 0 || N <= 0 || D <= 0 || Mpad <= 0 || (mode != 0 && mode != 1) || (mode == 1 && N < 2))
        return VITAE_ERR_INVALID_ARG;
    if ((long)B * N > Mpad || (Mpad & 63)) return VITAE_ERR_INVALID_ARG;
    if (((uintptr_t)dsel | (uintptr_t)dx | (uintptr_t)dx_bf16 | (uintptr_t)colsum) & 15) return VITAE_ERR_INVALID_ARG;
    if (D & 7) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const int D8 = D / 8;
    const long blocks = ((long)Mpad * D8 + 255) / 256;
    if (blocks > 0x7fffffffL) return VITAE_ERR_UNSUPPORTED_SHAPE;
    hipLaunchKernelGGL(token_select_bwd16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dsel, dx,
                       reinterpret_cast<__bf16*>(dx_bf16), colsum, B, N, Mpad, D8, mode, mode ? (float)(N - 1) : 1.0f);
    return vitae_launch_status();
}
