// The classifier end of fine-tuning (reference post_training_utils/fine_tune_epoch.py:58-63,104-145,366-376):
//   * vitae_cls_loss: class-weighted cross entropy on hard labels (torch.nn.CrossEntropyLoss(weight), mean reduction) or on soft
//     targets (utils/custom_loss.py:12-18) in ONE launch — loss, gradient of the logits, softmax, argmax and confusion counts;
//   * vitae_mixup_pairs / vitae_mixup_targets: batch-mode Mixup of the volumes (x <- lam x + (1 - lam) flip(x), both samples of a
//     pair in one pass) and of the labels (smoothed one-hot rows).
// The loss works on [B, C] logits with C = 2 and B of a few dozen: it is latency, not throughput.  One workgroup, one wave per
// row, everything between the fp32 inputs and the fp32 outputs in double, so every output is the float64 formula rounded once;
// sums run in a fixed order (lane partials in class order, a butterfly over the wave, the four waves in wave order): no float
// atomics, bitwise reproducible.  The mixup kernel is HBM bound: one 16-byte load and store per sample of a pair and lane.
#include "common.hpp"
#include "vitae_hip.h"

#include <math.h>

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);       // a + b on one side, b + a on the other: every lane ends equal
    return v;
}

// Sum over the 4 waves of a 256-thread block, in wave order; every thread gets the result.  `red` = 4 doubles of LDS.
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// hard mode (labels != NULL):  loss = sum_n w[y_n] (-logp[n, y_n]) / sum_n w[y_n],
//                              dlogits[n, c] = g w[y_n] (p[n, c] - [c == y_n]) / sum_m w[y_m]
// soft mode (targets != NULL): loss = sum_n sum_c -t[n, c] w[c] logp[n, c] / (C sum_c w[c]),
//                              dlogits[n, k] = g (p[n, k] sum_c t[n, c] w[c] - t[n, k] w[k]) / (C sum_c w[c])
__global__ __launch_bounds__(256) void cls_loss_kernel(const float* logits, long ld, const long long* labels, const float* targets,
                                                       const float* w, float g, float* loss, float* dlogits, float* probs, int* pred,
                                                       int* confusion, int B, int C) {
    __shared__ double red[4];
    __shared__ int bad_label;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool hard = labels != nullptr;
    if (tid == 0) bad_label = 0;

    // the denominator first: the gradient of every row needs it
    double part = 0.0;
    bool bad = false;
    if (hard) {
        for (int n = tid; n < B; n += 256) {
            const long long y = labels[n];
            if (y >= 0 && y < C) part += w ? (double)w[y] : 1.0;
            else if (y != -100) bad = true;                       // neither a class nor ignore_index: the loss becomes NaN
        }
    } else {
        for (int c = tid; c < C; c += 256) part += w ? (double)w[c] : 1.0;
    }
    double den = block_sum_d(part, red);
    if (!hard) den *= (double)C;
    if (bad) atomicOr(&bad_label, 1);

    double num = 0.0;                                             // this wave's rows, in row order
    for (int n = wave; n < B; n += 4) {
        const float* x = logits + (long)n * ld;
        // row maximum and its lowest index (torch.max)
        float m = -INFINITY;
        int am = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            const float v = x[c];
            if (c == lane || v > m) { m = v; am = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(m, o, 64);
            const int oa = __shfl_xor(am, o, 64);
            if (om > m || (om == m && oa < am)) { m = om; am = oa; }
        }
        m = __shfl(m, 0, 64);                                      // NaN logits order nothing: lane 0 (always a real column) decides
        am = min(__shfl(am, 0, 64), C - 1);
        const double md = (double)m;
        double s = 0.0;
        for (int c = lane; c < C; c += 64) s += exp((double)x[c] - md);
        const double lse = log(wave_sum_d(s));

        float* dl = dlogits ? dlogits + (long)n * C : nullptr;
        float* pr = probs ? probs + (long)n * C : nullptr;
        if (hard) {
            const long long y = labels[n];
            const bool valid = y >= 0 && y < C;
            const double wy = valid ? (w ? (double)w[y] : 1.0) : 0.0;
            if (valid) num += wy * -(((double)x[y] - md) - lse);
            const double scale = wy / den;
            for (int c = lane; c < C; c += 64) {
                const double p = exp(((double)x[c] - md) - lse);
                if (pr) pr[c] = (float)p;
                if (dl) dl[c] = valid ? g * (float)(scale * (p - (c == y ? 1.0 : 0.0))) : 0.f;
            }
            if (lane == 0 && confusion && valid) atomicAdd(&confusion[(long)am * C + y], 1);     // integer counts: exact in any order
        } else {
            const float* t = targets + (long)n * C;
            double tw = 0.0, nl = 0.0;
            for (int c = lane; c < C; c += 64) {
                const double twc = (double)t[c] * (w ? (double)w[c] : 1.0);
                tw += twc;
                nl -= twc * (((double)x[c] - md) - lse);
            }
            tw = wave_sum_d(tw);
            num += wave_sum_d(nl);
            for (int c = lane; c < C; c += 64) {
                const double p = exp(((double)x[c] - md) - lse);
                if (pr) pr[c] = (float)p;
                if (dl) dl[c] = g * (float)((p * tw - (double)t[c] * (w ? (double)w[c] : 1.0)) / den);
            }
        }
        if (lane == 0 && pred) pred[n] = am;
    }
    __syncthreads();
    if (lane == 0) red[wave] = num;
    __syncthreads();
    if (tid == 0) {
        const double total = ((red[0] + red[1]) + red[2]) + red[3];
        loss[0] = bad_label ? NAN : (float)(total / den);          // every row ignored: 0 / 0 = NaN, as torch
    }
}

__device__ __forceinline__ float mix1(float a, float b, double lam, double oml) { return (float)(lam * (double)a + oml * (double)b); }
__device__ __forceinline__ f32x4 mix1(f32x4 a, f32x4 b, double lam, double oml) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = mix1(a[e], b[e], lam, oml);
    return r;
}

// V = float or f32x4; nv = elements of V per sample.  Row r pairs sample r with sample B - 1 - r: both are read, both are
// written, by the same thread — so in place (dst == x) is safe.  The middle sample of an odd batch, and every sample when
// `identity` (lam == 1), are copied untouched (the host launches nothing for them in place).
template <typename V>
__global__ __launch_bounds__(256) void mixup_pairs_kernel(const V* x, V* dst, double lam, double oml, int identity, int B, long nv) {
    const int rows = (B + 1) / 2;
    const long step = (long)gridDim.x * 256;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const int j = B - 1 - r;
        const V* pa = x + (long)r * nv;
        const V* pb = x + (long)j * nv;
        V* oa = dst + (long)r * nv;
        V* ob = dst + (long)j * nv;
        if (r == j || identity) {
            if ((const V*)dst == x) continue;
            for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nv; c += step) {
                oa[c] = pa[c];
                if (r != j) ob[c] = pb[c];
            }
            continue;
        }
        for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nv; c += step) {
            const V a = pa[c], b = pb[c];
            oa[c] = mix1(a, b, lam, oml);
            ob[c] = mix1(b, a, lam, oml);
        }
    }
}

// out[i, c] = lam oh(y_i)[c] + (1 - lam) oh(y_{B-1-i})[c], oh(y)[c] = c == y ? on : off
__global__ __launch_bounds__(256) void mixup_targets_kernel(const long long* labels, float* out, double lam, double oml, double on,
                                                            double off, int B, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * C) return;
    const int n = (int)(i / C), c = (int)(i - (long)n * C);
    const long long ya = labels[n], yb = labels[B - 1 - n];
    float v = NAN;
    if (ya >= 0 && ya < C && yb >= 0 && yb < C) v = (float)(lam * (c == ya ? on : off) + oml * (c == yb ? on : off));
    out[i] = v;
}

}  // namespace

extern "C" int vitae_cls_loss(const float* logits, long ld, const long long* labels, const float* targets, const float* w, float g,
                              float* loss, float* dlogits, float* probs, int* pred, int* confusion, int B, int C, void* stream) {
    if (!logits || !loss || B < 1 || C < 1 || ld < C || (labels != nullptr) == (targets != nullptr) || (confusion && !labels))
        return VITAE_ERR_INVALID_ARG;
    if ((((uintptr_t)logits | (uintptr_t)targets | (uintptr_t)w | (uintptr_t)loss | (uintptr_t)dlogits | (uintptr_t)probs | (uintptr_t)pred |
          (uintptr_t)confusion) & 3) || ((uintptr_t)labels & 7))
        return VITAE_ERR_INVALID_ARG;
    if (C > 1024) return VITAE_ERR_UNSUPPORTED_SHAPE;
    hipLaunchKernelGGL(cls_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, ld, labels, targets, w, g, loss, dlogits,
                       probs, pred, confusion, B, C);
    return vitae_launch_status();
}

extern "C" int vitae_mixup_pairs(float* x, float* dst, double lam, int B, long n, void* stream) {
    if (!x || B < 1 || n < 1 || !(lam >= 0.0 && lam <= 1.0)) return VITAE_ERR_INVALID_ARG;
    if (!dst) dst = x;
    if (((uintptr_t)x | (uintptr_t)dst) & 3) return VITAE_ERR_INVALID_ARG;
    const uintptr_t xb = (uintptr_t)x, db = (uintptr_t)dst, bytes = (uintptr_t)B * (uintptr_t)n * 4;
    if (db != xb && db < xb + bytes && xb < db + bytes) return VITAE_ERR_INVALID_ARG;      // partial overlap
    const int identity = lam == 1.0;
    if (dst == x && (identity || B == 1)) return VITAE_OK;          // nothing changes: nothing is launched, x stays bit for bit
    const int rows = (B + 1) / 2;
    const bool vec = !(((uintptr_t)x | (uintptr_t)dst) & 15) && !(n & 3);
    const long nv = vec ? n / 4 : n;
    const dim3 grid((unsigned)(nv < 2048L * 256 ? cdiv(nv, 256) : 2048), (unsigned)(rows < 65535 ? rows : 65535));
    if (vec)
        hipLaunchKernelGGL(mixup_pairs_kernel<f32x4>, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const f32x4*>(x),
                           reinterpret_cast<f32x4*>(dst), lam, 1.0 - lam, identity, B, nv);
    else
        hipLaunchKernelGGL(mixup_pairs_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)x, dst, lam, 1.0 - lam,
                           identity, B, nv);
    return vitae_launch_status();
}

extern "C" int vitae_mixup_targets(const long long* labels, float* out, double lam, double smoothing, int B, int C, void* stream) {
    if (!labels || !out || B < 1 || C < 1 || !(lam >= 0.0 && lam <= 1.0) || !(smoothing >= 0.0 && smoothing <= 1.0))
        return VITAE_ERR_INVALID_ARG;
    if (((uintptr_t)labels & 7) || ((uintptr_t)out & 3)) return VITAE_ERR_INVALID_ARG;
    const double off = smoothing / C, on = 1.0 - smoothing + off;
    hipLaunchKernelGGL(mixup_targets_kernel, dim3(cdiv((long)B * C, 256)), dim3(256), 0, (hipStream_t)stream, labels, out, lam,
                       1.0 - lam, on, off, B, C);
    return vitae_launch_status();
}
