// RandomBlur of the fine-tuning scripts (post_training_utils/fine_tune_epoch.py:248-255: tio.RandomBlur() between RandomAffine and
// RandomNoise) as a batch kernel: every item gets its own Gaussian on every axis.  torchio blurs each channel with
// scipy.ndimage.gaussian_filter(channel, std): one axis after the other (0, 1, 2), radius int(4 sigma + 0.5), weights normalised in
// float64, border mode 'reflect' (d c b a | a b c d | d c b a).  The host (utils/augment.py) computes the taps in float64, rounds
// them once to fp32 and uploads them with the radii; the kernels below are deterministic functions of (input, table).
//
// The radius is a run-time value, uniform within a workgroup (a workgroup belongs to one item), so the window lives in LDS:
//   blur_z_kernel    stages a [planes of one z-tile + 2 rz] x 64-column slab of one (b, c) volume ("column" = 64 consecutive voxels of
//                    the flattened (y, x) plane) and blurs along z; lane = column, so consecutive lanes read consecutive words;
//   blur_yx_kernel   stages a band of rows of one (b, c, z) plane with its reflected halo on both axes, blurs along y into a second
//                    LDS image, then along x from that image to global memory; lane = x in both passes.
// Every source index goes through reflect(), which lands in [0, n) for every int, so no load leaves the volume whatever the table
// holds; the radii read from the table are clamped to the maxima the launcher sized the LDS from.
// A tap is broadcast from the lane that holds it (v_readlane, the tap index is uniform): no memory traffic in the inner loop.
// The sum starts from the first product and adds the others in index order with fmaf: an axis of radius 0 is 1.0f * v, an exact
// copy of every bit pattern.
#include "common.hpp"
#include "vitae_hip.h"

namespace {

constexpr int BLUR_COLS = 64;     // blur_z_kernel: columns a slab (one per lane)
constexpr int BLUR_ZT = VITAE_BLUR_TILE_Z, BLUR_TY = VITAE_BLUR_TILE_Y, BLUR_TX = VITAE_BLUR_TILE_X;

// scipy's 'reflect' (half-sample symmetric), periodic with period 2n: valid for every i and every n >= 1
__device__ __forceinline__ int reflect(int i, int n) {
    const int p = 2 * n;
    int j = i % p;
    if (j < 0) j += p;
    return j >= n ? p - 1 - j : j;
}

// lane k of the wave holds tap k of the table row (k < VITAE_BLUR_MAX_TAPS <= 64)
__device__ __forceinline__ float load_taps(const float* __restrict__ row) {
    const int lane = threadIdx.x & 63;
    return lane < VITAE_BLUR_MAX_TAPS ? row[lane] : 0.f;
}
__device__ __forceinline__ float tap(float wv, int k) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv), k));
}
// sum_{k=0..2r} w[k] s[k * stride]: the first product starts the sum, the others join it in index order.  Four LDS reads are issued
// ahead of their four fmaf (hipcc does not unroll a loop around v_readlane when asked to); the chain keeps its order.
__device__ __forceinline__ float window_sum(float wv, const float* s, int stride, int r) {
    float acc = tap(wv, 0) * s[0];
    int k = 1;
    for (; k + 3 <= 2 * r; k += 4) {
        const float v0 = s[k * stride], v1 = s[(k + 1) * stride], v2 = s[(k + 2) * stride], v3 = s[(k + 3) * stride];
        acc = fmaf(tap(wv, k), v0, acc);
        acc = fmaf(tap(wv, k + 1), v1, acc);
        acc = fmaf(tap(wv, k + 2), v2, acc);
        acc = fmaf(tap(wv, k + 3), v3, acc);
    }
    for (; k <= 2 * r; ++k) acc = fmaf(tap(wv, k), s[k * stride], acc);
    return acc;
}

// out[z] = sum_k w[k] in[reflect(z + k - r)] along the slowest axis.  grid: (column slabs x z-tiles, C, B)
__global__ __launch_bounds__(256) void blur_z_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                     const float* __restrict__ taps, const int* __restrict__ radii, int rcap, int C,
                                                     int Lz, long plane, int nslab) {
    extern __shared__ float lds[];                      // [zt + 2 r][BLUR_COLS]
    const int b = blockIdx.z, c = blockIdx.y;
    const int slab = blockIdx.x % nslab, zt = blockIdx.x / nslab;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = min(max(radii[3 * b + 0], 0), rcap);
    const float wv = load_taps(taps + (long)(3 * b + 0) * VITAE_BLUR_MAX_TAPS);
    const int z0 = zt * BLUR_ZT, nz = min(BLUR_ZT, Lz - z0);
    const long col = (long)slab * BLUR_COLS + lane;
    const long base = ((long)b * C + c) * Lz * plane;
    if (col < plane) {
        for (int i = wave; i < nz + 2 * r; i += 4) lds[i * BLUR_COLS + lane] = in[base + (long)reflect(z0 - r + i, Lz) * plane + col];
    }
    __syncthreads();
    if (col >= plane) return;
    for (int i = wave; i < nz; i += 4) {
        out[base + (long)(z0 + i) * plane + col] = window_sum(wv, lds + i * BLUR_COLS + lane, BLUR_COLS, r);
    }
}

// y, then x, on a band of rows of one plane.  grid: (x-tiles x y-tiles x Lz, C, B)
__global__ __launch_bounds__(256) void blur_yx_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                      const float* __restrict__ taps, const int* __restrict__ radii, int rycap,
                                                      int rxcap, int C, int Lz, int Hy, int Wx, int nxt, int nyt) {
    extern __shared__ float lds[];                      // s1 [ny + 2 ry][w1], then s2 [ny][w1];  w1 = nx + 2 rx
    const int b = blockIdx.z, c = blockIdx.y;
    const int xt = blockIdx.x % nxt, yt = (blockIdx.x / nxt) % nyt, z = blockIdx.x / (nxt * nyt);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ry = min(max(radii[3 * b + 1], 0), rycap), rx = min(max(radii[3 * b + 2], 0), rxcap);
    const float wy = load_taps(taps + (long)(3 * b + 1) * VITAE_BLUR_MAX_TAPS);
    const float wx = load_taps(taps + (long)(3 * b + 2) * VITAE_BLUR_MAX_TAPS);
    const int y0 = yt * BLUR_TY, ny = min(BLUR_TY, Hy - y0);
    const int x0 = xt * BLUR_TX, nx = min(BLUR_TX, Wx - x0);
    const int w1 = nx + 2 * rx;
    float* s1 = lds;
    float* s2 = lds + (ny + 2 * ry) * w1;
    const long base = (((long)b * C + c) * Lz + z) * (long)Hy * Wx;
    for (int i = wave; i < ny + 2 * ry; i += 4) {
        const float* row = in + base + (long)reflect(y0 - ry + i, Hy) * Wx;
        for (int j = lane; j < w1; j += 64) s1[i * w1 + j] = row[reflect(x0 - rx + j, Wx)];
    }
    __syncthreads();
    for (int i = wave; i < ny; i += 4) {
        for (int j = lane; j < w1; j += 64) s2[i * w1 + j] = window_sum(wy, s1 + i * w1 + j, w1, ry);
    }
    __syncthreads();
    for (int i = wave; i < ny; i += 4) {
        float* orow = out + base + (long)(y0 + i) * Wx + x0;
        for (int j = lane; j < nx; j += 64) orow[j] = window_sum(wx, s2 + i * w1 + j, 1, rx);
    }
}

}  // namespace

extern "C" int vitae_random_blur(const float* x, float* tmp, float* y, const float* taps, const int* radii, const int* radii_host,
                                 int B, int C, int Lz, int Hy, int Wx, void* stream) {
    if (!x || !y || !taps || !radii || !radii_host || x == y || B <= 0 || C <= 0 || Lz <= 0 || Hy <= 0 || Wx <= 0)
        return VITAE_ERR_INVALID_ARG;
    if (B > 65535 || C > 65535 || max(Lz, max(Hy, Wx)) > (1 << 30)) return VITAE_ERR_UNSUPPORTED_SHAPE;   // reflect() doubles an extent
    int rz = 0, ry = 0, rx = 0;
    for (int b = 0; b < B; ++b) {
        const int* r = radii_host + 3 * b;
        if (r[0] < 0 || r[1] < 0 || r[2] < 0) return VITAE_ERR_INVALID_ARG;
        rz = max(rz, r[0]); ry = max(ry, r[1]); rx = max(rx, r[2]);
    }
    if (max(rz, max(ry, rx)) > VITAE_BLUR_MAX_RADIUS) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const bool pass_z = rz > 0, pass_yx = ry > 0 || rx > 0;
    if (pass_z && pass_yx && (!tmp || tmp == x || tmp == y)) return VITAE_ERR_INVALID_ARG;
    const long plane = (long)Hy * Wx;
    const int nslab = cdiv(plane, BLUR_COLS), nzt = cdiv(Lz, BLUR_ZT);
    const int nxt = cdiv(Wx, BLUR_TX), nyt = cdiv(Hy, BLUR_TY);
    if ((long)nslab * nzt > 0x7fffffffL || (long)nxt * nyt * Lz > 0x7fffffffL) return VITAE_ERR_UNSUPPORTED_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    if (!pass_z && !pass_yx) {      // every axis of every item is an exact copy: one copy, not three passes
        return hipMemcpyAsync(y, x, (size_t)B * C * Lz * plane * sizeof(float), hipMemcpyDeviceToDevice, st) == hipSuccess
                   ? VITAE_OK : VITAE_ERR_LAUNCH;
    }
    // LDS from the batch's largest radii: at most (128 + 32) x 64 floats = 40 KB and (64 + 32) x (128 + 32) floats = 60 KB at
    // the cap, below the 64 KB a launch may ask for without raising the limit
    const float* src = x;
    if (pass_z) {
        float* dst = pass_yx ? tmp : y;
        const size_t lds = (size_t)(min(BLUR_ZT, Lz) + 2 * rz) * BLUR_COLS * sizeof(float);
        hipLaunchKernelGGL(blur_z_kernel, dim3(nslab * nzt, C, B), dim3(256), lds, st, src, dst, taps, radii, rz, C, Lz, plane, nslab);
        src = dst;
    }
    if (pass_yx) {
        const int nyM = min(BLUR_TY, Hy), w1M = min(BLUR_TX, Wx) + 2 * rx;
        const size_t lds = (size_t)(2 * nyM + 2 * ry) * w1M * sizeof(float);
        hipLaunchKernelGGL(blur_yx_kernel, dim3(nxt * nyt * Lz, C, B), dim3(256), lds, st, src, y, taps, radii, ry, rx, C, Lz, Hy, Wx,
                           nxt, nyt);
    }
    return vitae_launch_status();
}
