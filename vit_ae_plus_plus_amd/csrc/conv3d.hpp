// What the two convolution units share (conv3d.hip: bf16 operands; conv3d_x3.hip: fp32 sources split into bf16 hi + lo): the
// geometry and its refusals, the coordinate rule of one axis, the two-level accumulation and the ordered sum of the weight
// gradient's partials.  Everything is internal to a unit (anonymous namespace): each unit compiles its own copy.
#pragma once
#include "common.hpp"
#include "vitae_hip.h"

#include <limits.h>
#include <initializer_list>

namespace {

constexpr int KSTEP = VITAE_CONV3D_K_STEP;
constexpr int MAX_TAPS = 7 * 7 * 7;
constexpr int WCHUNK = VITAE_CONV3D_WGRAD_CHUNK;
// Two-level accumulation: the MFMA chain runs FLUSH k-steps (128 k-values) in fp32 and is then added to a double total.  One fp32
// chain over the stem's 1372 steps (all products of one sign) was 18 ulp off in the worst element, 4.6 x torch's blocked fp32 sum.
constexpr int FLUSH = 8;

__device__ __forceinline__ void flush_acc(f32x16& acc, double (&tot)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) { tot[i] += (double)acc[i]; acc[i] = 0.f; }
}

struct ConvGeo {
    int N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw;
    int Do, Ho, Wo, taps;
    long M, V;          // output rows N Do Ho Wo, input voxels N D H W
    long K;             // taps * Cin
};

// VITAE_OK or the refusal; fills g
inline int conv_geo(ConvGeo& g, int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return VITAE_ERR_INVALID_ARG;
    if (kd < 1 || kh < 1 || kw < 1 || kd > 7 || kh > 7 || kw > 7) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (sd < 1 || sh < 1 || sw < 1 || sd > 2 || sh > 2 || sw > 2) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (pd < 0 || ph < 0 || pw < 0 || pd >= kd || ph >= kh || pw >= kw) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (Cout & 3) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (D + 2 * pd < kd || H + 2 * ph < kh || W + 2 * pw < kw) return VITAE_ERR_UNSUPPORTED_SHAPE;      // an output extent <= 0
    g = ConvGeo{N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw};
    g.Do = (D + 2 * pd - kd) / sd + 1; g.Ho = (H + 2 * ph - kh) / sh + 1; g.Wo = (W + 2 * pw - kw) / sw + 1;
    g.taps = kd * kh * kw;
    g.M = (long)N * g.Do * g.Ho * g.Wo;
    g.V = (long)N * D * H * W;
    g.K = (long)g.taps * Cin;
    const long lim = (long)INT_MAX - 256;
    if (g.M > lim || g.V > lim || g.K > lim || (long)g.taps * Cout > lim) return VITAE_ERR_UNSUPPORTED_SHAPE;
    return VITAE_OK;
}

inline long kpad(long K) { return (K + KSTEP - 1) / KSTEP * KSTEP; }
inline int shift_of(int c) { return (c & (c - 1)) == 0 ? __builtin_ctz(c) : -1; }
inline bool aligned16(std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs) if ((uintptr_t)q & 15) return false;
    return true;
}

// One axis of the coordinate rule.  Forward: source = row * stride - pad + tap.  Input gradient: t = voxel + pad - tap must be a
// non-negative multiple of the stride (1 or 2) and t / stride an existing output position.
template <bool BWD>
__device__ __forceinline__ bool conv_axis(int base, int tap, int stride, int extent, int& c) {
    if (!BWD) { c = base + tap; return c >= 0 && c < extent; }
    const int t = base - tap;
    c = t >> (stride - 1);
    return t >= 0 && (t & (stride - 1)) == 0 && c < extent;
}

// the weight gradient's partials in chunk order -> torch's [Cout, Cin, taps]
__global__ __launch_bounds__(256) void conv3d_wgrad_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, int chunks, int Cout, int Cin,
                                                               int taps, int accumulate) {
    const long total = (long)Cout * Cin * taps;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;              // over [co][k = tap Cin + ci]: coalesced partial reads
    if (i >= total) return;
    double sd = 0.;
    for (int z = 0; z < chunks; ++z) sd += (double)ws[(long)z * total + i];
    const float s = (float)sd;
    const int K = taps * Cin;
    const int co = (int)(i / K), k = (int)(i % K), tap = k / Cin, ci = k % Cin;
    const long o = ((long)co * Cin + ci) * taps + tap;
    dw[o] = accumulate ? dw[o] + s : s;
}

}  // namespace
