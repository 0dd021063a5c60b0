// Loss chain of the ViT-AE++ objective (reference ops K14-K21 and K24):
//   masked-voxel reconstruction MSE   model/vit_autoenc.py:226-227 (target = patchify(imgs), :100-113)
//   unpatchify(pred)                  model/vit_autoenc.py:115-128, 221
//   Gaussian blur of the target       model/model_utils/gaussian_filter.py:16-26 (11 taps, zero pad)
//   3D Sobel magnitude, channel sum   model/model_utils/sobel_filter.py:37-45
//   edge-map MSE                      model/vit_autoenc.py:224-225
//   SimSiam cosine loss               utils/train_one_epoch.py:113-114
// All HBM-bound streaming / stencil work in fp32.  `pred` is addressed through (row stride P, batch
// stride) so the decoder output with its cls row ([B, L+1, P]) is consumed in place.  Scalar sums go
// to a double accumulator block `acc` (VITAE_ACC_*), finalised by tiny kernels; upstream gradient
// multipliers are read from the device-resident `hp` block (VITAE_HP_*) so captured graphs can be
// replayed while edge_map_weight / accum scaling change.
#include <cstdlib>
#include "common.hpp"
#include "vitae_hip.h"
#ifndef VITAE_BLUR_ROWS
#define VITAE_BLUR_ROWS 32
#endif

namespace {

struct VolGeom {
    int C, Lz, Hy, Wx, p, g1, g2, L;
    long P, pred_bstride;   // pred element (b, l, e) at pred[b*pred_bstride + l*P + e]
};

__device__ __forceinline__ long vol_index(const VolGeom& g, int b, int l, int e) {
    // patchify order inside a patch: e = ((r*p + s)*p + q)*C + c   (vit_autoenc.py:111)
    const int c = e % g.C;
    int rem = e / g.C;
    const int q = rem % g.p; rem /= g.p;
    const int s = rem % g.p;
    const int r = rem / g.p;
    const int gl = l / (g.g1 * g.g2), gh = (l / g.g2) % g.g1, gw = l % g.g2;
    return (((long)(b * g.C + c) * g.Lz + gl * g.p + r) * g.Hy + gh * g.p + s) * g.Wx + gw * g.p + q;
}

// ---------------------------------------------------------------- masked reconstruction loss
__global__ __launch_bounds__(256) void recon_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ imgs,
                                                        const float* __restrict__ mask, double* __restrict__ acc,
                                                        VolGeom g) {
    __shared__ float red[4];
    const int l = blockIdx.x, b = blockIdx.y;
    if (mask[(long)b * g.L + l] == 0.f) return;
    const float* prow = pred + (long)b * g.pred_bstride + (long)l * g.P;
    float s = 0.f;
    for (int e = threadIdx.x; e < g.P; e += 256) {
        const float d = prow[e] - imgs[vol_index(g, b, l, e)];
        s += d * d;
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) atomicAdd(acc + VITAE_ACC_RECON, (double)(s / (float)g.P));
}

// dpred = 2 (pred - target) * mask / (P * mask.sum()) * g_recon
__global__ __launch_bounds__(256) void recon_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ imgs,
                                                        const float* __restrict__ mask, const float* __restrict__ hp,
                                                        float* __restrict__ dpred, float inv_p_masksum, VolGeom g) {
    const int l = blockIdx.x, b = blockIdx.y;
    const long off = (long)b * g.pred_bstride + (long)l * g.P;
    float* drow = dpred + off;
    if (mask[(long)b * g.L + l] == 0.f) {
        for (int e = threadIdx.x; e < g.P; e += 256) drow[e] = 0.f;
        return;
    }
    const float coef = 2.f * hp[VITAE_HP_G_RECON] * inv_p_masksum;
    const float* prow = pred + off;
    for (int e = threadIdx.x; e < g.P; e += 256) drow[e] = coef * (prow[e] - imgs[vol_index(g, b, l, e)]);
}

// ---------------------------------------------------------------- unpatchify(pred) -> volume
__global__ __launch_bounds__(256) void unpatchify_kernel(const float* __restrict__ pred, float* __restrict__ vol, VolGeom g) {
    const int l = blockIdx.x, b = blockIdx.y;
    const float* prow = pred + (long)b * g.pred_bstride + (long)l * g.P;
    for (int e = threadIdx.x; e < g.P; e += 256) vol[vol_index(g, b, l, e)] = prow[e];
}

// ---------------------------------------------------------------- separable Gaussian blur (one axis)
struct Taps { float k[VITAE_MAX_TAPS]; int n; };

__global__ __launch_bounds__(256) void blur_axis_kernel(const float* __restrict__ in, float* __restrict__ out, long total,
                                                        int len, long inner, Taps t) {
    const int rad = t.n / 2;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int pos = (int)((idx / inner) % len);
        float s = 0.f;
        for (int i = 0; i < t.n; ++i) {
            const int pp = pos + i - rad;
            if (pp >= 0 && pp < len) s += t.k[i] * in[idx + (long)(i - rad) * inner];
        }
        out[idx] = s;
    }
}

// ---------------------------------------------------------------- 3D Sobel
// Cross-correlation with the three kernels of sobel_filter.py:12-31 (zero padding 1):
//   g0 = s(z) s(y) d(x),  g1 = s(z) e(y) s(x),  g2 = e(z) s(y) s(x),  s=[1,2,1], d=[1,0,-1], e=[-1,0,1]
__device__ __forceinline__ void sobel_at(const float* __restrict__ v, int z, int y, int x, int Lz, int Hy, int Wx,
                                         float& g0, float& g1, float& g2) {
    g0 = g1 = g2 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int zz = z + a - 1;
        if (zz < 0 || zz >= Lz) continue;
        const float sa = a == 1 ? 2.f : 1.f, ea = (float)(a - 1);
#pragma unroll
        for (int bb = 0; bb < 3; ++bb) {
            const int yy = y + bb - 1;
            if (yy < 0 || yy >= Hy) continue;
            const float sb = bb == 1 ? 2.f : 1.f, eb = (float)(bb - 1);
            const float* row = v + ((long)zz * Hy + yy) * Wx;
            const float xm = x > 0 ? row[x - 1] : 0.f;
            const float x0 = row[x];
            const float xp = x + 1 < Wx ? row[x + 1] : 0.f;
            const float sx = xm + 2.f * x0 + xp;   // s along x
            const float dx = xm - xp;              // d = [1, 0, -1] along x
            g0 += sa * sb * dx;
            g1 += sa * eb * sx;
            g2 += ea * sb * sx;
        }
    }
}

// E[b, z, y, x] = sum_c |grad|;  optionally accumulates sum (E - E_ref)^2 into acc[VITAE_ACC_EDGE].
__global__ __launch_bounds__(256) void sobel_mag_kernel(const float* __restrict__ vol, float* __restrict__ E,
                                                        const float* __restrict__ E_ref, double* __restrict__ acc,
                                                        int B, int C, int Lz, int Hy, int Wx) {
    __shared__ float red[4];
    const long V = (long)Lz * Hy * Wx, total = (long)B * V;
    float sq = 0.f;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int b = (int)(idx / V);
        const long r = idx % V;
        const int x = (int)(r % Wx), y = (int)((r / Wx) % Hy), z = (int)(r / ((long)Wx * Hy));
        float e = 0.f;
        for (int c = 0; c < C; ++c) {
            float g0, g1, g2;
            sobel_at(vol + ((long)b * C + c) * V, z, y, x, Lz, Hy, Wx, g0, g1, g2);
            e += sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
        }
        E[idx] = e;
        if (E_ref) { const float d = e - E_ref[idx]; sq += d * d; }
    }
    if (E_ref) {
        sq = block_sum_256(sq, red);
        if (threadIdx.x == 0) atomicAdd(acc + VITAE_ACC_EDGE, (double)sq);
    }
}

// dG[b, c, a, voxel] = dE * g_a / |g|,  dE = 2 (E_pred - E_tgt) * g_edge / (B*V).
// |g| == 0 gives 0/0 = NaN exactly like sqrt's backward in the reference.
__global__ __launch_bounds__(256) void sobel_bwd_components_kernel(const float* __restrict__ vol, const float* __restrict__ Ep,
                                                                   const float* __restrict__ Et, const float* __restrict__ hp,
                                                                   float* __restrict__ dG, float inv_count, int B, int C,
                                                                   int Lz, int Hy, int Wx) {
    const long V = (long)Lz * Hy * Wx, total = (long)B * V;
    const float coef = 2.f * hp[VITAE_HP_G_EDGE] * inv_count;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int b = (int)(idx / V);
        const long r = idx % V;
        const int x = (int)(r % Wx), y = (int)((r / Wx) % Hy), z = (int)(r / ((long)Wx * Hy));
        const float dE = coef * (Ep[idx] - Et[idx]);
        for (int c = 0; c < C; ++c) {
            float g0, g1, g2;
            sobel_at(vol + ((long)b * C + c) * V, z, y, x, Lz, Hy, Wx, g0, g1, g2);
            const float m = sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
            const float f = dE / m;
            float* o = dG + (((long)b * C + c) * 3) * V + r;
            o[0] = f * g0; o[V] = f * g1; o[2 * V] = f * g2;
        }
    }
}

// dvol[u] = sum_a sum_o w_a[o] * dG_a[u - o + 1]  (transpose of the correlation), scattered straight
// into dpred (patchify order) with +=.
__global__ __launch_bounds__(256) void sobel_bwd_scatter_kernel(const float* __restrict__ dG, float* __restrict__ dpred,
                                                                __bf16* __restrict__ dpred16, int B, VolGeom g) {
    const int Lz = g.Lz, Hy = g.Hy, Wx = g.Wx, C = g.C, p = g.p;
    const long V = (long)Lz * Hy * Wx, total = (long)B * V;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int b = (int)(idx / V);
        const long r = idx % V;
        const int x = (int)(r % Wx), y = (int)((r / Wx) % Hy), z = (int)(r / ((long)Wx * Hy));
        const int l = ((z / p) * g.g1 + y / p) * g.g2 + x / p;
        const int e0 = (((z % p) * p + y % p) * p + x % p) * C;
        const long doff = (long)b * g.pred_bstride + (long)l * g.P + e0;
        float* drow = dpred + doff;
        for (int c = 0; c < C; ++c) {
            const float* d0 = dG + (((long)b * C + c) * 3) * V;
            float acc = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int zz = z - a + 1;
                if (zz < 0 || zz >= Lz) continue;
                const float sa = a == 1 ? 2.f : 1.f, ea = (float)(a - 1);
#pragma unroll
                for (int bb = 0; bb < 3; ++bb) {
                    const int yy = y - bb + 1;
                    if (yy < 0 || yy >= Hy) continue;
                    const float sb = bb == 1 ? 2.f : 1.f, eb = (float)(bb - 1);
                    const long ro = ((long)zz * Hy + yy) * Wx;
                    // o = 0,1,2 along x reads dG at x+1, x, x-1 with weights (d: 1,0,-1 ; s: 1,2,1)
                    const bool hp_ = x + 1 < Wx, hm = x > 0;
                    const float a0p = hp_ ? d0[ro + x + 1] : 0.f, a0m = hm ? d0[ro + x - 1] : 0.f;
                    const float a1p = hp_ ? d0[V + ro + x + 1] : 0.f, a10 = d0[V + ro + x], a1m = hm ? d0[V + ro + x - 1] : 0.f;
                    const float a2p = hp_ ? d0[2 * V + ro + x + 1] : 0.f, a20 = d0[2 * V + ro + x], a2m = hm ? d0[2 * V + ro + x - 1] : 0.f;
                    acc += sa * sb * (a0p - a0m);
                    acc += sa * eb * (a1p + 2.f * a10 + a1m);
                    acc += ea * sb * (a2p + 2.f * a20 + a2m);
                }
            }
            const float fin = drow[c] + acc;
            drow[c] = fin;
            if (dpred16) dpred16[doff + c] = (__bf16)fin;
        }
    }
}

// ---------------------------------------------------------------- LDS-tiled variants (the ones the step uses)
// Blur, x and y axes in one pass: a block owns a band of TY rows of one (b,c,z) plane, stages the band plus
// RAD halo rows (zero padded in x and y) in LDS, blurs along x into a second LDS buffer, then along y.
// Summation order per axis equals blur_axis_kernel's (out-of-range taps add an exact 0).
template <int RAD>
__device__ __forceinline__ void blur_xy_body(const dim3 blockIdx_, const float* __restrict__ in, float* __restrict__ out, int Hy, int Wx,
                                                      int TY, Taps t) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    static_assert((2 * RAD + 2) % 4 == 0, "row stride must stay a multiple of 4 floats for the 16-byte LDS accesses");
    constexpr int NT = 2 * RAD + 1, XB = 4;   // XB outputs per thread along x share their NT + XB - 1 inputs
    const int rows = TY + 2 * RAD;
    const int Wp = (Wx + XB - 1) / XB * XB, stride = Wp + 2 * RAD + 2;   // +2: de-phase consecutive rows' banks
    float* a = sm;                    // [rows][stride]  input, zero padded
    float* m = sm + rows * stride;    // [rows][Wp]      blurred along x
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y0 = blockIdx_.x * TY;
    const float* src = in + (long)blockIdx_.y * Hy * Wx;
    float* dst = out + (long)blockIdx_.y * Hy * Wx;
    for (int r = wave; r < rows; r += 4) {
        const int yy = y0 - RAD + r;
        const bool rin = yy >= 0 && yy < Hy;
        for (int xs = lane; xs < stride; xs += 64) {
            const int xx = xs - RAD;
            a[r * stride + xs] = (rin && xx >= 0 && xx < Wx) ? src[(long)yy * Wx + xx] : 0.f;
        }
    }
    __syncthreads();
    const int groups = Wp / XB;
    for (int w = threadIdx.x; w < rows * groups; w += 256) {
        const int r = w / groups, x = (w - r * groups) * XB;
        const float* row = a + r * stride + x;
        // 16-byte LDS reads (x and stride are multiples of 4, the row has 2 RAD + 2 floats of slack behind Wp): with
        // 4-byte reads at a 4-float lane stride every bank served 4 lanes (68 % of this kernel's LDS cycles were conflicts)
        constexpr int NV4 = (NT + XB - 1 + 3) / 4;
        static_assert(4 * NV4 <= XB + 2 * RAD + 2, "the padded row must cover the widened read");
        float v[4 * NV4];
#pragma unroll
        for (int i = 0; i < NV4; ++i) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(row + 4 * i);
            v[4 * i] = q[0]; v[4 * i + 1] = q[1]; v[4 * i + 2] = q[2]; v[4 * i + 3] = q[3];
        }
        f32x4 res;
#pragma unroll
        for (int o = 0; o < XB; ++o) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < NT; ++i) acc += t.k[i] * v[o + i];
            res[o] = acc;
        }
        *reinterpret_cast<f32x4*>(&m[r * Wp + x]) = res;
    }
    __syncthreads();
    // y: one thread per (column, half band); inputs fetched once into registers
    constexpr int YB = 11;
    const int segs = (TY + YB - 1) / YB;
    for (int w = threadIdx.x; w < Wx * segs; w += 256) {
        const int sgm = w / Wx, x = w - sgm * Wx, r0 = sgm * YB;
        float v[YB + NT - 1];
#pragma unroll
        for (int i = 0; i < YB + NT - 1; ++i) v[i] = (r0 + i < rows) ? m[(r0 + i) * Wp + x] : 0.f;
#pragma unroll
        for (int o = 0; o < YB; ++o) {
            const int yy = y0 + r0 + o;
            if (r0 + o < TY && yy < Hy) {
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < NT; ++i) acc += t.k[i] * v[o + i];
                dst[(long)yy * Wx + x] = acc;
            }
        }
    }
}

// Blur along z: one thread per (y,x) column and z chunk; the ZC + 2 RAD inputs are fetched up front (all loads
// in flight together) and each output is a static-index dot product in registers.
template <int RAD, int ZC>
__device__ __forceinline__ void blur_z_body(const dim3 blockIdx_, const float* __restrict__ in, float* __restrict__ out, int Lz, long plane,
                                                     Taps t) {
    const long pos = (long)blockIdx_.x * 256 + threadIdx.x;
    if (pos >= plane) return;
    const int z0 = blockIdx_.y * ZC;
    const float* src = in + (long)blockIdx_.z * Lz * plane + pos;
    float* dst = out + (long)blockIdx_.z * Lz * plane + pos;
    float v[ZC + 2 * RAD];
#pragma unroll
    for (int i = 0; i < ZC + 2 * RAD; ++i) {
        const int zz = z0 - RAD + i;
        v[i] = (zz >= 0 && zz < Lz) ? src[(long)zz * plane] : 0.f;
    }
#pragma unroll
    for (int o = 0; o < ZC; ++o) {
        if (z0 + o >= Lz) break;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 2 * RAD + 1; ++i) acc += t.k[i] * v[o + i];
        dst[(long)(z0 + o) * plane] = acc;
    }
}

// Sobel stencils, separable form.  In-plane partials of one z plane at (y, x):
//   A = s(y) d(x),  Bp = e(y) s(x),  Cp = s(y) s(x);   g0 = s(z) A, g1 = s(z) Bp, g2 = e(z) Cp.
// `row` points at the LDS element (y-1, x-1) of the plane, `rs` is the LDS row stride.
__device__ __forceinline__ void sobel_plane(const float* row, int rs, float& A, float& Bp, float& Cp) {
    const float a0 = row[0], a1 = row[1], a2 = row[2];
    const float b0 = row[rs], b1 = row[rs + 1], b2 = row[rs + 2];
    const float c0 = row[2 * rs], c1 = row[2 * rs + 1], c2 = row[2 * rs + 2];
    const float sa = a0 + 2.f * a1 + a2, sb = b0 + 2.f * b1 + b2, sc = c0 + 2.f * c1 + c2;
    const float da = a0 - a2, db = b0 - b2, dc = c0 - c2;
    A = da + 2.f * db + dc;
    Bp = sc - sa;
    Cp = sa + 2.f * sb + sc;
}

constexpr int TZ = 8, TY_ = 8, TX = 32;                       // output tile of the Sobel kernels (z, y, x)

// E = sum_c |grad vol_c| on a TZ x TY x TX tile: the tile plus a 1-voxel halo of one channel sits in LDS, each
// thread owns one (y, x) column and marches along z with a 3-plane register ring of the in-plane partials.
__device__ __forceinline__ void sobel_mag_tiled_body(const dim3 blockIdx_, const float* __restrict__ vol, float* __restrict__ E,
                                                              const float* __restrict__ E_ref, double* __restrict__ acc,
                                                              int C, int Lz, int Hy, int Wx, int xtiles) {
    constexpr int RZ = TZ + 2, RY = TY_ + 2, RX = TX + 2;
    __shared__ float sv[RZ * RY * RX];
    __shared__ float red[4];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x0 = (blockIdx_.x % xtiles) * TX, y0 = (blockIdx_.x / xtiles) * TY_, z0 = blockIdx_.y * TZ, b = blockIdx_.z;
    const long V = (long)Lz * Hy * Wx;
    float e[TZ];
#pragma unroll
    for (int i = 0; i < TZ; ++i) e[i] = 0.f;
    constexpr int NLD = (RZ * RY * RX + 255) / 256;
    float pre[NLD];
    auto fetch = [&](int c) {
        const float* src = vol + ((long)b * C + c) * V;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = threadIdx.x + k * 256;
            const int xx = idx % RX, r = idx / RX, yy = r % RY, zz = r / RY;
            const int gx = x0 - 1 + xx, gy = y0 - 1 + yy, gz = z0 - 1 + zz;
            const bool in = idx < RZ * RY * RX && gx >= 0 && gx < Wx && gy >= 0 && gy < Hy && gz >= 0 && gz < Lz;
            pre[k] = in ? src[((long)gz * Hy + gy) * Wx + gx] : 0.f;
        }
    };
    fetch(0);
    for (int c = 0; c < C; ++c) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int idx = threadIdx.x + k * 256;
            if (idx < RZ * RY * RX) sv[idx] = pre[k];
        }
        __syncthreads();
        if (c + 1 < C) fetch(c + 1);     // next channel's loads fly underneath this channel's stencil
        float A0, B0, C0, A1, B1, C1, A2, B2, C2;
        sobel_plane(sv + (0 * RY + ty) * RX + tx, RX, A0, B0, C0);
        sobel_plane(sv + (1 * RY + ty) * RX + tx, RX, A1, B1, C1);
#pragma unroll
        for (int zz = 2; zz < RZ; ++zz) {
            sobel_plane(sv + (zz * RY + ty) * RX + tx, RX, A2, B2, C2);
            const float g0 = A0 + 2.f * A1 + A2, g1 = B0 + 2.f * B1 + B2, g2 = C2 - C0;
            e[zz - 2] += sqrtf(g0 * g0 + g1 * g1 + g2 * g2);
            A0 = A1; B0 = B1; C0 = C1; A1 = A2; B1 = B2; C1 = C2;
        }
    }
    float sq = 0.f;
    const int x = x0 + tx, y = y0 + ty;
    if (x < Wx && y < Hy) {
        float er[TZ];
#pragma unroll
        for (int i = 0; i < TZ; ++i) {
            const long o = (long)b * V + ((long)min(z0 + i, Lz - 1) * Hy + y) * Wx + x;
            er[i] = E_ref ? E_ref[o] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < TZ; ++i) {
            const int z = z0 + i;
            if (z < Lz) {
                E[(long)b * V + ((long)z * Hy + y) * Wx + x] = e[i];
                const float d = e[i] - er[i];
                sq += d * d;
            }
        }
    }
    if (E_ref) {
        sq = block_sum_256(sq, red);
        if (threadIdx.x == 0) atomicAdd(acc + VITAE_ACC_EDGE, (double)sq);
    }
}

// Grid-stride forms of the three target-branch kernels (the branch only depends on the input volume and runs on a
// side stream under the transformer).  A cap on their grids was measured: capping to 256-1024
// workgroups does NOT help the step (5.73-5.78 ms vs 5.69 uncapped) because these kernels are latency-bound per
// workgroup and slow down more than they give back, so the launchers give them the full virtual grid.
template <int RAD>
__global__ __launch_bounds__(256) void blur_xy_kernel(const float* __restrict__ in, float* __restrict__ out, int Hy, int Wx,
                                                      int TY, Taps t, int nbx, int total) {
    for (int v = blockIdx.x; v < total; v += gridDim.x) {
        blur_xy_body<RAD>(dim3(v % nbx, v / nbx, 0), in, out, Hy, Wx, TY, t);
        __syncthreads();
    }
}

template <int RAD, int ZC>
__global__ __launch_bounds__(256) void blur_z_kernel(const float* __restrict__ in, float* __restrict__ out, int Lz, long plane,
                                                     Taps t, int nbx, int nby, int total) {
    for (int v = blockIdx.x; v < total; v += gridDim.x)
        blur_z_body<RAD, ZC>(dim3(v % nbx, (v / nbx) % nby, v / (nbx * nby)), in, out, Lz, plane, t);
}

__global__ __launch_bounds__(256) void sobel_mag_tiled_kernel(const float* __restrict__ vol, float* __restrict__ E,
                                                              const float* __restrict__ E_ref, double* __restrict__ acc,
                                                              int C, int Lz, int Hy, int Wx, int xtiles, int nbx, int nby,
                                                              int total) {
    for (int v = blockIdx.x; v < total; v += gridDim.x) {
        sobel_mag_tiled_body(dim3(v % nbx, (v / nbx) % nby, v / (nbx * nby)), vol, E, E_ref, acc, C, Lz, Hy, Wx, xtiles);
        __syncthreads();
    }
}

// Forward loss terms on the prediction in ONE pass over it (C = 4): reads pred in patchify order (one 16-byte
// load per voxel = its four channels), writes the unpatchified volume for the backward, the Sobel edge map, and
// accumulates both loss sums:   acc[RECON] += sum_masked (pred - img)^2 / P,   acc[EDGE] += sum (E_pred - E_tgt)^2.
// Replaces recon_fwd + unpatchify + sobel_mag_tiled (three passes over the 57 MB prediction).
__global__ __launch_bounds__(256) void loss_fwd_fused_kernel(const float* __restrict__ pred, const float* __restrict__ imgs,
                                                             const float* __restrict__ mask, const float* __restrict__ Et,
                                                             float* __restrict__ pvol, float* __restrict__ Ep,
                                                             double* __restrict__ acc, int xtiles, VolGeom g) {
    constexpr int RZ = TZ + 2, RY = TY_ + 2, RX = TX + 2, NV = RZ * RY * RX, NLD = (NV + 255) / 256;
    __shared__ f32x4 sv[NV];
    __shared__ float red[4];
    const int Lz = g.Lz, Hy = g.Hy, Wx = g.Wx, p = g.p;
    const long V = (long)Lz * Hy * Wx;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x0 = (blockIdx.x % xtiles) * TX, y0 = (blockIdx.x / xtiles) * TY_, z0 = blockIdx.y * TZ, b = blockIdx.z;
    const float* pb = pred + (long)b * g.pred_bstride;
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int idx = threadIdx.x + k * 256;
        if (idx < NV) {
            const int xx = idx % RX, r = idx / RX, yy = r % RY, zz = r / RY;
            const int gx = x0 - 1 + xx, gy = y0 - 1 + yy, gz = z0 - 1 + zz;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gx >= 0 && gx < Wx && gy >= 0 && gy < Hy && gz >= 0 && gz < Lz) {
                const int l = ((gz / p) * g.g1 + gy / p) * g.g2 + gx / p;
                const int e0 = (((gz % p) * p + gy % p) * p + gx % p) * 4;
                v = *reinterpret_cast<const f32x4*>(pb + (long)l * g.P + e0);
            }
            sv[idx] = v;
        }
    }
    // this thread's column: image values and mask flags of its TZ voxels (issued before the barrier)
    const int x = x0 + tx, y = y0 + ty;
    const bool live = x < Wx && y < Hy;
    const int xc = min(x, Wx - 1), yc = min(y, Hy - 1);
    float im[4][TZ], mk[TZ], et[TZ];
#pragma unroll
    for (int tz = 0; tz < TZ; ++tz) {
        const int z = min(z0 + tz, Lz - 1);
        const int l = ((z / p) * g.g1 + yc / p) * g.g2 + xc / p;
        mk[tz] = mask[(long)b * g.L + l];
        const long o = ((long)z * Hy + yc) * Wx + xc;
        et[tz] = Et[(long)b * V + o];
#pragma unroll
        for (int c = 0; c < 4; ++c) im[c][tz] = imgs[((long)b * 4 + c) * V + o];
    }
    __syncthreads();
    auto plane = [&](int zz, f32x4& A, f32x4& Bp, f32x4& Cp) {
        const f32x4* row = sv + (zz * RY + ty) * RX + tx;
        const f32x4 a0 = row[0], a1 = row[1], a2 = row[2];
        const f32x4 b0 = row[RX], b1 = row[RX + 1], b2 = row[RX + 2];
        const f32x4 c0 = row[2 * RX], c1 = row[2 * RX + 1], c2 = row[2 * RX + 2];
        const f32x4 sa = a0 + 2.f * a1 + a2, sb = b0 + 2.f * b1 + b2, sc = c0 + 2.f * c1 + c2;
        const f32x4 da = a0 - a2, db = b0 - b2, dc = c0 - c2;
        A = da + 2.f * db + dc;
        Bp = sc - sa;
        Cp = sa + 2.f * sb + sc;
    };
    f32x4 A0, B0, C0, A1, B1, C1, A2, B2, C2;
    plane(0, A0, B0, C0);
    plane(1, A1, B1, C1);
    float sq = 0.f, rc = 0.f;
#pragma unroll
    for (int zz = 2; zz < RZ; ++zz) {
        plane(zz, A2, B2, C2);
        const int tz = zz - 2, z = z0 + tz;
        const f32x4 g0 = A0 + 2.f * A1 + A2, g1 = B0 + 2.f * B1 + B2, g2 = C2 - C0;
        const f32x4 m2 = g0 * g0 + g1 * g1 + g2 * g2;
        const float e = sqrtf(m2[0]) + sqrtf(m2[1]) + sqrtf(m2[2]) + sqrtf(m2[3]);
        if (live && z < Lz) {
            const long o = ((long)z * Hy + y) * Wx + x;
            Ep[(long)b * V + o] = e;
            const float d = e - et[tz];
            sq += d * d;
            const f32x4 pv = sv[((tz + 1) * RY + ty + 1) * RX + tx + 1];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                pvol[((long)b * 4 + c) * V + o] = pv[c];
                if (mk[tz] != 0.f) { const float dd = pv[c] - im[c][tz]; rc += dd * dd; }
            }
        }
        A0 = A1; B0 = B1; C0 = C1; A1 = A2; B1 = B2; C1 = C2;
    }
    sq = block_sum_256(sq, red);
    __syncthreads();
    rc = block_sum_256(rc, red);
    if (threadIdx.x == 0) {
        atomicAdd(acc + VITAE_ACC_EDGE, (double)sq);
        atomicAdd(acc + VITAE_ACC_RECON, (double)(rc / (float)g.P));
    }
}

// Whole loss backward in one pass over the volume:
//   dpred = mask * 2 g_recon (pred - img) / (P mask.sum())  +  d(edge mse)/d pred          (fp32 and optional bf16)
// Per tile and channel: pred_vol tile + 2-voxel halo -> LDS; Sobel components on tile + 1 halo, scaled by
// dE / |g| (dE = 2 g_edge (E_pred - E_tgt) / (B V), exact 0 outside the volume; |g| == 0 gives NaN like the
// reference's sqrt backward) -> three LDS arrays; transposed (flipped) separable stencils over those -> dvol.
// All C channels of a voxel are adjacent in patchify order, so they are collected in registers and stored as
// one vector per voxel.
// one LDS-DMA lane-piece: 16 bytes (WIDE) or 4 (the size operand must be a literal)
template <bool WIDE> __device__ __forceinline__ void lds_dma(const float* src, float* dst);
template <> __device__ __forceinline__ void lds_dma<true>(const float* src, float* dst) {
    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}
template <> __device__ __forceinline__ void lds_dma<false>(const float* src, float* dst) {
    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
}

// ROW16: the pred_vol tile goes HBM -> LDS in 16-byte pieces of x-rows (tile x-extent + a 4-voxel halo on each side so that
// every piece starts 16-byte aligned: 40 floats = 10 pieces per row, 6 DMA instructions per thread and channel) instead of one
// float per lane (21 instructions per thread and channel, 256 bytes per wave instruction: the texture addresser, not HBM, bounded
// the kernel).  Needs Wx % 4 == 0.
template <int CH, bool ROW16>
__global__ __launch_bounds__(256, 2) void loss_bwd_fused_kernel(const float* __restrict__ pvol, const float* __restrict__ imgs,
                                                             const float* __restrict__ mask, const float* __restrict__ Ep,
                                                             const float* __restrict__ Et, const float* __restrict__ hp,
                                                             float* __restrict__ dpred, __bf16* __restrict__ dpred16,
                                                             float* __restrict__ nonfinite, float inv_count,
                                                             float inv_p_masksum, int xtiles, VolGeom g) {
    constexpr int VZ = TZ + 4, VY = TY_ + 4, VX = ROW16 ? TX + 8 : TX + 4;      // pred_vol region (halo 2; ROW16: x halo 4)
    constexpr int XH = ROW16 ? 4 : 2;                          // x halo of the staged region
    constexpr int GZ = TZ + 2, GY = TY_ + 2, GX = TX + 2;      // dG region (halo 1)
    constexpr int NCOL = GY * GX, NPASS = (NCOL + 255) / 256;
    __shared__ __attribute__((aligned(16))) float sv[VZ * VY * VX];
    __shared__ float sg[3][GZ * GY * GX];
    const int Lz = g.Lz, Hy = g.Hy, Wx = g.Wx;
    const long V = (long)Lz * Hy * Wx;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int x0 = (blockIdx.x % xtiles) * TX, y0 = (blockIdx.x / xtiles) * TY_, z0 = blockIdx.y * TZ, b = blockIdx.z;
    const float ce = 2.f * hp[VITAE_HP_G_EDGE] * inv_count, cr = 2.f * hp[VITAE_HP_G_RECON] * inv_p_masksum;

    // dE at this thread's dG columns (same for every channel); one bit per column voxel says "inside the volume" (a NaN
    // in dE is data: a non-finite prediction has to reach dpred, it must not read as "outside")
    float de[NPASS][GZ];
    unsigned inbits = 0u;
    static_assert(NPASS * GZ <= 32, "one bit per dG voxel of a thread");
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
        const int col = threadIdx.x + ps * 256;
        const int cx = col % GX, cy = col / GX;
        const int gx = x0 - 1 + cx, gy = y0 - 1 + cy;
        const bool cin = col < NCOL && gx >= 0 && gx < Wx && gy >= 0 && gy < Hy;
#pragma unroll
        for (int k = 0; k < GZ; ++k) {
            const int gz = z0 - 1 + k;
            float v = 0.f;
            if (cin && gz >= 0 && gz < Lz) {
                const long o = (long)b * V + ((long)gz * Hy + gy) * Wx + gx;
                v = ce * (Ep[o] - Et[o]);
                inbits |= 1u << (ps * GZ + k);
            }
            de[ps][k] = v;
        }
    }
    float o[CH][TZ];
    const int x = x0 + tx, y = y0 + ty;
    const bool live = x < Wx && y < Hy;
    const int xc = min(x, Wx - 1), yc = min(y, Hy - 1);
    // reconstruction-term inputs of this thread's TZ voxels: mask flags now, image values per channel (below)
    float im[TZ];
    unsigned mkbits = 0u;
#pragma unroll
    for (int tz = 0; tz < TZ; ++tz) {
        const int z = min(z0 + tz, Lz - 1);
        const int l = ((z / g.p) * g.g1 + yc / g.p) * g.g2 + xc / g.p;
        mkbits |= (mask[(long)b * g.L + l] != 0.f ? 1u : 0u) << tz;
    }
    // The pred_vol tile (+ 2-voxel halo) of a channel goes HBM -> LDS by DMA (global_load_lds, 4 B per lane, LDS
    // destination lane-linear = the flat tile index): the element offsets are computed once and reused for every
    // channel (the index arithmetic was a third of the kernel's instructions), no registers hold data in flight,
    // and the next channel's tile is fetched underneath the transposed stencils.  Out-of-volume elements are zeroed
    // once and never written again (their lanes are masked out of the DMA).
    constexpr int NPIECE = ROW16 ? VZ * VY * (VX / 4) : VZ * VY * VX;       // DMA lane-pieces of one channel's region
    constexpr int NLD = (NPIECE + 255) / 256;
    int off[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int idx = threadIdx.x + k * 256;
        if constexpr (ROW16) {
            const int ch = idx % (VX / 4), r = idx / (VX / 4), yy = r % VY, zz = r / VY;
            const int gx = x0 - XH + 4 * ch, gy = y0 - 2 + yy, gz = z0 - 2 + zz;
            const bool in = idx < NPIECE && gx >= 0 && gx + 3 < Wx && gy >= 0 && gy < Hy && gz >= 0 && gz < Lz;   // Wx % 4 == 0: all or nothing
            off[k] = in ? (gz * Hy + gy) * Wx + gx : -1;
            if (!in && idx < NPIECE) *reinterpret_cast<float4*>(sv + idx * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const int xx = idx % VX, r = idx / VX, yy = r % VY, zz = r / VY;
            const int gx = x0 - 2 + xx, gy = y0 - 2 + yy, gz = z0 - 2 + zz;
            const bool in = idx < NPIECE && gx >= 0 && gx < Wx && gy >= 0 && gy < Hy && gz >= 0 && gz < Lz;
            off[k] = in ? (gz * Hy + gy) * Wx + gx : -1;
            if (!in && idx < NPIECE) sv[idx] = 0.f;
        }
    }
    const int wave_base = (threadIdx.x >> 6) * 64;
    auto fetch = [&](int c) {
        const float* src = pvol + ((long)b * g.C + c) * V;
#pragma unroll
        for (int k = 0; k < NLD; ++k)
            if (off[k] >= 0) lds_dma<ROW16>(src + off[k], sv + (k * 256 + wave_base) * (ROW16 ? 4 : 1));
    };
    fetch(0);
    for (int c = 0; c < CH; ++c) {
#pragma unroll
        for (int tz = 0; tz < TZ; ++tz)
            im[tz] = imgs[((long)b * g.C + c) * V + ((long)min(z0 + tz, Lz - 1) * Hy + yc) * Wx + xc];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's DMA pieces of channel c landed
        __syncthreads();                                     // ... everyone's; last channel's sg readers are done
        float pvc[TZ];
#pragma unroll
        for (int tz = 0; tz < TZ; ++tz) pvc[tz] = sv[((tz + 2) * VY + ty + 2) * VX + tx + XH];
        // ---- dG on the halo-1 region, one (y, x) column per thread (and a second one for the first threads)
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int col = threadIdx.x + ps * 256;
            if (col < NCOL) {
                const int cx = col % GX, cy = col / GX;
                const float* base = sv + cy * VX + cx + (XH - 2);        // region (vz, cy .. cy+2, cx .. cx+2)
                float A0, B0, C0, A1, B1, C1, A2, B2, C2;
                sobel_plane(base, VX, A0, B0, C0);
                sobel_plane(base + VY * VX, VX, A1, B1, C1);
#pragma unroll
                for (int vz = 2; vz < VZ; ++vz) {
                    sobel_plane(base + vz * VY * VX, VX, A2, B2, C2);
                    const float g0 = A0 + 2.f * A1 + A2, g1 = B0 + 2.f * B1 + B2, g2 = C2 - C0;
                    const float d = de[ps][vz - 2];
                    const bool in = (inbits >> (ps * GZ + vz - 2)) & 1u;
                    const float f = d * __builtin_amdgcn_rsqf(g0 * g0 + g1 * g1 + g2 * g2);   // |g| = 0 -> inf -> NaN below
                    const int gi = ((vz - 2) * GY + cy) * GX + cx;
                    sg[0][gi] = in ? f * g0 : 0.f;
                    sg[1][gi] = in ? f * g1 : 0.f;
                    sg[2][gi] = in ? f * g2 : 0.f;
                    A0 = A1; B0 = B1; C0 = C1; A1 = A2; B1 = B2; C1 = C2;
                }
            }
        }
        __syncthreads();
        if (c + 1 < CH) fetch(c + 1);    // sv is free: next channel's tile flies underneath the transposed stencils
        // ---- transposed stencils: dvol = s(z)[ s(y)e(x) G0 + d(y)s(x) G1 ] + d(z) s(y)s(x) G2
        float Q0, P0, Q1, P1, Q2, P2;
        auto plane = [&](int gz, float& Q, float& P) {
            const float* r0 = &sg[0][(gz * GY + ty) * GX + tx];
            const float* r1 = &sg[1][(gz * GY + ty) * GX + tx];
            const float* r2 = &sg[2][(gz * GY + ty) * GX + tx];
            const float q0 = (r0[2] - r0[0]) + 2.f * (r0[GX + 2] - r0[GX]) + (r0[2 * GX + 2] - r0[2 * GX]);
            const float s1a = r1[0] + 2.f * r1[1] + r1[2], s1c = r1[2 * GX] + 2.f * r1[2 * GX + 1] + r1[2 * GX + 2];
            const float s2a = r2[0] + 2.f * r2[1] + r2[2], s2b = r2[GX] + 2.f * r2[GX + 1] + r2[GX + 2],
                        s2c = r2[2 * GX] + 2.f * r2[2 * GX + 1] + r2[2 * GX + 2];
            Q = q0 + (s1a - s1c);
            P = s2a + 2.f * s2b + s2c;
        };
        plane(0, Q0, P0);
        plane(1, Q1, P1);
#pragma unroll
        for (int gz = 2; gz < GZ; ++gz) {
            plane(gz, Q2, P2);
            const int tz = gz - 2;
            float val = (Q0 + 2.f * Q1 + Q2) + (P0 - P2);
            if ((mkbits >> tz) & 1u) val = cr * (pvc[tz] - im[tz]) + val;
            o[c][tz] = val;
            Q0 = Q1; P0 = P1; Q1 = Q2; P1 = P2;
        }
    }
    if (!live) return;
    bool bad = false;
#pragma unroll
    for (int tz = 0; tz < TZ; ++tz) {
        const int z = z0 + tz;
        if (z >= Lz) break;
#pragma unroll
        for (int c = 0; c < CH; ++c) bad |= !(fabsf(o[c][tz]) <= 3.4028234e38f);   // NaN or inf
        const int p = g.p;
        const int l = ((z / p) * g.g1 + y / p) * g.g2 + x / p;
        const int e0 = (((z % p) * p + y % p) * p + x % p) * CH;
        const long doff = (long)b * g.pred_bstride + (long)l * g.P + e0;
        if constexpr (CH == 4) {
            *reinterpret_cast<float4*>(dpred + doff) = make_float4(o[0][tz], o[1][tz], o[2][tz], o[3][tz]);
            if (dpred16) {
                typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
                bf4 h = {(__bf16)o[0][tz], (__bf16)o[1][tz], (__bf16)o[2][tz], (__bf16)o[3][tz]};
                *reinterpret_cast<bf4*>(dpred16 + doff) = h;
            }
        } else {
#pragma unroll
            for (int c = 0; c < CH; ++c) {
                dpred[doff + c] = o[c][tz];
                if (dpred16) dpred16[doff + c] = (__bf16)o[c][tz];
            }
        }
    }
    if (bad && nonfinite) *nonfinite = __builtin_nanf("");   // benign race: every writer stores the same value
}

// ---------------------------------------------------------------- scalar finalisation
// out = [loss, raw_edge_mse, recon, percep(=0)]   (vit_autoenc.py:231-232)
__global__ void loss_finalize_kernel(const double* __restrict__ acc, const float* __restrict__ hp, float* __restrict__ out,
                                     float inv_masksum, float inv_edge_count) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float recon = (float)(acc[VITAE_ACC_RECON]) * inv_masksum;
    const float edge = (float)(acc[VITAE_ACC_EDGE] * (double)inv_edge_count);
    out[0] = hp[VITAE_HP_EDGE_W] * edge + recon + 0.f;
    out[1] = edge;
    out[2] = recon;
    out[3] = 0.f;
}

// ---------------------------------------------------------------- SimSiam cosine loss
// One wave per row: cos(p, z) = <p/max(|p|,eps), z/max(|z|,eps)>  (nn.CosineSimilarity, eps 1e-8)
__global__ __launch_bounds__(256) void cosine_fwd_kernel(const float* __restrict__ p1, const float* __restrict__ z2,
                                                         const float* __restrict__ p2, const float* __restrict__ z1,
                                                         double* __restrict__ acc, int R, int D, float eps) {
    // ONE atomic per workgroup (round 5: one double atomic per row and pair — 7040 on the same address at batch 32 — serialised in L2:
    // 49 us for 22 MB)
    __shared__ double red[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double csum = 0.0;
    for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
            const float* p = (pair == 0 ? p1 : p2) + (long)row * D;
            const float* z = (pair == 0 ? z2 : z1) + (long)row * D;
            float dot = 0.f, pp = 0.f, zz = 0.f;
            for (int d = lane; d < D; d += 64) { const float a = p[d], b = z[d]; dot += a * b; pp += a * a; zz += b * b; }
            dot = wave_sum(dot); pp = wave_sum(pp); zz = wave_sum(zz);
            csum += (double)(dot / (fmaxf(sqrtf(pp), eps) * fmaxf(sqrtf(zz), eps)));
        }
    }
    if (lane == 0) red[wave] = csum;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc + VITAE_ACC_COS, (red[0] + red[1]) + (red[2] + red[3]));
}

// The same for D = 256 NV with everything a row needs in flight at once (round 6: the scalar form above walks a row in twelve
// dependent 4-byte steps per pair, the pairs one after the other — 14 us for 220 x 768 at batch 4, on the step's one queue), and the
// scalar result written by the LAST workgroup to arrive (acc[VITAE_ACC_TICKET_C]; it leaves the ticket at zero) instead of by a
// launch of its own.
template <int NV>
__global__ __launch_bounds__(256) void cosine_fwd_vec_kernel(const float* __restrict__ p1, const float* __restrict__ z2,
                                                             const float* __restrict__ p2, const float* __restrict__ z1,
                                                             double* __restrict__ acc, const float* __restrict__ hp,
                                                             float* __restrict__ out, float inv_rows, int R, float eps) {
    constexpr int D = 256 * NV;
    __shared__ double red[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double csum = 0.0;
    for (int row = blockIdx.x * 4 + wave; row < R; row += gridDim.x * 4) {
        f32x4 a[2][NV], b[2][NV];
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
            const f32x4* p = reinterpret_cast<const f32x4*>((pair == 0 ? p1 : p2) + (long)row * D);
            const f32x4* z = reinterpret_cast<const f32x4*>((pair == 0 ? z2 : z1) + (long)row * D);
#pragma unroll
            for (int i = 0; i < NV; ++i) { a[pair][i] = p[lane + 64 * i]; b[pair][i] = z[lane + 64 * i]; }
        }
#pragma unroll
        for (int pair = 0; pair < 2; ++pair) {
            float dot = 0.f, pp = 0.f, zz = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float x = a[pair][i][e], y = b[pair][i][e]; dot += x * y; pp += x * x; zz += y * y; }
            dot = wave_sum(dot); pp = wave_sum(pp); zz = wave_sum(zz);
            csum += (double)(dot / (fmaxf(sqrtf(pp), eps) * fmaxf(sqrtf(zz), eps)));
        }
    }
    if (lane == 0) red[wave] = csum;
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicAdd(acc + VITAE_ACC_COS, (red[0] + red[1]) + (red[2] + red[3]));
        __threadfence();
        unsigned* ticket = reinterpret_cast<unsigned*>(acc + VITAE_ACC_TICKET_C);
        if (atomicAdd(ticket, 1u) == gridDim.x - 1) {
            __threadfence();
            const double total = atomicAdd(acc + VITAE_ACC_COS, 0.0);      // (device-scope read of what every workgroup added)
            out[0] = hp[VITAE_HP_CONTR_W] * (float)(-0.5 * total * (double)inv_rows);
            atomicExch(ticket, 0u);
        }
    }
}

// contr = contr_w * (-(mean cos(p1,z2) + mean cos(p2,z1)) / 2)
__global__ void cosine_finalize_kernel(const double* __restrict__ acc, const float* __restrict__ hp, float* __restrict__ out, float inv_rows) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    out[0] = hp[VITAE_HP_CONTR_W] * (float)(-0.5 * acc[VITAE_ACC_COS] * (double)inv_rows);
}

// dp = g_contr * (-0.5 / R) * ( z/(|p||z|) - cos * p/|p|^2 ), norms clamped at eps; the second term only where |p| >= eps
__global__ __launch_bounds__(256) void cosine_bwd_kernel(const float* __restrict__ p1, const float* __restrict__ z2,
                                                         const float* __restrict__ p2, const float* __restrict__ z1,
                                                         const float* __restrict__ hp, float* __restrict__ dp1,
                                                         float* __restrict__ dp2, __bf16* __restrict__ dp1_16,
                                                         __bf16* __restrict__ dp2_16, int R, int D, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;
    const float coef = hp[VITAE_HP_G_CONTR] * (-0.5f / (float)R);
#pragma unroll
    for (int pair = 0; pair < 2; ++pair) {
        const float* p = (pair == 0 ? p1 : p2) + (long)row * D;
        const float* z = (pair == 0 ? z2 : z1) + (long)row * D;
        float* dp = (pair == 0 ? dp1 : dp2);
        __bf16* dp16 = (pair == 0 ? dp1_16 : dp2_16);
        if (dp) dp += (long)row * D;
        if (dp16) dp16 += (long)row * D;
        float dot = 0.f, pp = 0.f, zz = 0.f;
        for (int d = lane; d < D; d += 64) { const float a = p[d], b = z[d]; dot += a * b; pp += a * a; zz += b * b; }
        dot = wave_sum(dot); pp = wave_sum(pp); zz = wave_sum(zz);
        const float rp = sqrtf(pp);
        const float np = fmaxf(rp, eps), nz = fmaxf(sqrtf(zz), eps);
        const float c = dot / (np * nz);
        // below the clamp the norm IS the constant eps: cos = <p, z> / (eps |z|) has no p / |p|^2 term (clamp_min passes no gradient)
        const float k1 = coef / (np * nz), k2 = rp >= eps ? coef * c / (np * np) : 0.f;
        for (int d = lane; d < D; d += 64) {
            const float v = k1 * z[d] - k2 * p[d];
            if (dp) dp[d] = v;
            if (dp16) dp16[d] = (__bf16)v;             // the predictor's backward GEMMs read this copy (no cast launch in between)
        }
    }
}

inline VolGeom make_geom(int C, int Lz, int Hy, int Wx, int p, long pred_bstride) {
    VolGeom g;
    g.C = C; g.Lz = Lz; g.Hy = Hy; g.Wx = Wx; g.p = p;
    g.g1 = Hy / p; g.g2 = Wx / p; g.L = (Lz / p) * g.g1 * g.g2;
    g.P = (long)p * p * p * C; g.pred_bstride = pred_bstride;
    return g;
}

// what every launcher of the chain refuses BEFORE its first launch (make_geom and the kernels divide by p; a grid of (L, B)
// workgroups holds at most 65535 batch elements)
inline bool bad_extents(int B, int C, int Lz, int Hy, int Wx) { return B <= 0 || C <= 0 || Lz <= 0 || Hy <= 0 || Wx <= 0; }
inline bool bad_patches(int Lz, int Hy, int Wx, int p) { return p <= 0 || Lz % p || Hy % p || Wx % p; }

inline int stream_blocks(long total) {
    long b = (total + 255) / 256;
    return (int)(b > 4096 ? 4096 : b);
}

}  // namespace

extern "C" int vitae_recon_loss_fwd(const float* pred, long pred_bstride, const float* imgs, const float* mask,
                                    double* acc, int B, int C, int Lz, int Hy, int Wx, int p, void* stream) {
    if (!pred || !imgs || !mask || !acc || bad_extents(B, C, Lz, Hy, Wx) || B > 65535 || bad_patches(Lz, Hy, Wx, p)) return VITAE_ERR_INVALID_ARG;
    VolGeom g = make_geom(C, Lz, Hy, Wx, p, pred_bstride);
    hipLaunchKernelGGL(recon_fwd_kernel, dim3(g.L, B), dim3(256), 0, (hipStream_t)stream, pred, imgs, mask, acc, g);
    return vitae_launch_status();
}

extern "C" int vitae_recon_loss_bwd(const float* pred, long pred_bstride, const float* imgs, const float* mask,
                                    const float* hp, float* dpred, float mask_sum, int B, int C, int Lz, int Hy,
                                    int Wx, int p, void* stream) {
    if (!pred || !imgs || !mask || !hp || !dpred || bad_extents(B, C, Lz, Hy, Wx) || B > 65535 || bad_patches(Lz, Hy, Wx, p) || !(mask_sum > 0.f))
        return VITAE_ERR_INVALID_ARG;
    VolGeom g = make_geom(C, Lz, Hy, Wx, p, pred_bstride);
    const float inv = 1.0f / ((float)g.P * mask_sum);
    hipLaunchKernelGGL(recon_bwd_kernel, dim3(g.L, B), dim3(256), 0, (hipStream_t)stream, pred, imgs, mask, hp, dpred,
                       inv, g);
    return vitae_launch_status();
}

extern "C" int vitae_unpatchify(const float* pred, long pred_bstride, float* vol, int B, int C, int Lz, int Hy, int Wx,
                                int p, void* stream) {
    if (!pred || !vol || bad_extents(B, C, Lz, Hy, Wx) || B > 65535 || bad_patches(Lz, Hy, Wx, p)) return VITAE_ERR_INVALID_ARG;
    VolGeom g = make_geom(C, Lz, Hy, Wx, p, pred_bstride);
    hipLaunchKernelGGL(unpatchify_kernel, dim3(g.L, B), dim3(256), 0, (hipStream_t)stream, pred, vol, g);
    return vitae_launch_status();
}

extern "C" int vitae_gauss_blur_fwd(const float* vol, float* tmp, float* out, const float* taps_host, int ntaps,
                                    int BC, int Lz, int Hy, int Wx, void* stream) {
    if (!vol || !tmp || !out || !taps_host || ntaps <= 0 || ntaps > VITAE_MAX_TAPS || !(ntaps & 1) || bad_extents(BC, 1, Lz, Hy, Wx))
        return VITAE_ERR_INVALID_ARG;
    Taps t; t.n = ntaps;
    for (int i = 0; i < ntaps; ++i) t.k[i] = taps_host[i];
    const long total = (long)BC * Lz * Hy * Wx;
    const int blocks = stream_blocks(total);
    hipStream_t st = (hipStream_t)stream;
    // x, then y, then z (exact-arithmetic equal to the dense k (x) k (x) k kernel of the reference)
    if (ntaps == 11 && Wx <= 384 && (long)Lz * BC <= 65535) {
        constexpr int RAD = 5, ROWS = VITAE_BLUR_ROWS, ZC = 32;   // 48- and 64-row bands measured slower (98 / 100 vs 86 us)
        const int TY = ROWS - 2 * RAD;
        const int Wp = (Wx + 3) / 4 * 4;
        const size_t lds = (size_t)ROWS * (2 * Wp + 2 * RAD + 2) * sizeof(float);
        const int nbx = cdiv(Hy, TY), tot_xy = nbx * Lz * BC;
        if (lds > 64 * 1024) {   // Wx > 250 (99,840 bytes at 384): past the default dynamic-LDS limit of a launch
            static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&blur_xy_kernel<RAD>),
                                                                hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024);
            (void)attr;
        }
        hipLaunchKernelGGL(blur_xy_kernel<RAD>, dim3(tot_xy), dim3(256), lds, st, vol, tmp, Hy, Wx, TY, t, nbx,
                           tot_xy);
        const long plane = (long)Hy * Wx;
        const int zx = cdiv(plane, 256), zy = cdiv(Lz, ZC), tot_z = zx * zy * BC;
        hipLaunchKernelGGL((blur_z_kernel<RAD, ZC>), dim3(tot_z), dim3(256), 0, st, tmp, out, Lz, plane, t, zx, zy,
                           tot_z);
        return vitae_launch_status();
    }
    hipLaunchKernelGGL(blur_axis_kernel, dim3(blocks), dim3(256), 0, st, vol, out, total, Wx, 1L, t);
    hipLaunchKernelGGL(blur_axis_kernel, dim3(blocks), dim3(256), 0, st, out, tmp, total, Hy, (long)Wx, t);
    hipLaunchKernelGGL(blur_axis_kernel, dim3(blocks), dim3(256), 0, st, tmp, out, total, Lz, (long)Wx * Hy, t);
    return vitae_launch_status();
}

extern "C" int vitae_sobel_edge_fwd(const float* vol, float* edge, const float* edge_ref, double* acc, int B, int C,
                                    int Lz, int Hy, int Wx, void* stream) {
    if (!vol || !edge || bad_extents(B, C, Lz, Hy, Wx) || (edge_ref && !acc)) return VITAE_ERR_INVALID_ARG;
    const int xt = cdiv(Wx, TX), yt = cdiv(Hy, TY_), zt = cdiv(Lz, TZ);
    if (zt <= 65535 && B <= 65535) {
        const int tot = xt * yt * zt * B;
        hipLaunchKernelGGL(sobel_mag_tiled_kernel, dim3(tot), dim3(256), 0, (hipStream_t)stream, vol, edge,
                           edge_ref, acc, C, Lz, Hy, Wx, xt, xt * yt, zt, tot);
        return vitae_launch_status();
    }
    const long total = (long)B * Lz * Hy * Wx;
    hipLaunchKernelGGL(sobel_mag_kernel, dim3(stream_blocks(total)), dim3(256), 0, (hipStream_t)stream, vol, edge,
                       edge_ref, acc, B, C, Lz, Hy, Wx);
    return vitae_launch_status();
}

extern "C" int vitae_sobel_edge_bwd(const float* pred_vol, const float* edge_pred, const float* edge_tgt,
                                    const float* hp, float* dG_ws, float* dpred, void* dpred_bf16, long pred_bstride, int B, int C,
                                    int Lz, int Hy, int Wx, int p, void* stream) {
    if (!pred_vol || !edge_pred || !edge_tgt || !hp || !dG_ws || !dpred || bad_extents(B, C, Lz, Hy, Wx) || bad_patches(Lz, Hy, Wx, p))
        return VITAE_ERR_INVALID_ARG;
    const long total = (long)B * Lz * Hy * Wx;
    VolGeom g = make_geom(C, Lz, Hy, Wx, p, pred_bstride);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sobel_bwd_components_kernel, dim3(stream_blocks(total)), dim3(256), 0, st, pred_vol, edge_pred,
                       edge_tgt, hp, dG_ws, 1.0f / (float)total, B, C, Lz, Hy, Wx);
    hipLaunchKernelGGL(sobel_bwd_scatter_kernel, dim3(stream_blocks(total)), dim3(256), 0, st, dG_ws, dpred,
                       reinterpret_cast<__bf16*>(dpred_bf16), B, g);
    return vitae_launch_status();
}

extern "C" int vitae_loss_fwd_fused(const float* pred, long pred_bstride, const float* imgs, const float* mask,
                                    const float* edge_tgt, float* pred_vol, float* edge_pred, double* acc, int B, int C,
                                    int Lz, int Hy, int Wx, int p, void* stream) {
    if (!pred || !imgs || !mask || !edge_tgt || !pred_vol || !edge_pred || !acc || bad_extents(B, C, Lz, Hy, Wx) || B > 65535 ||
        bad_patches(Lz, Hy, Wx, p))
        return VITAE_ERR_INVALID_ARG;
    VolGeom g = make_geom(C, Lz, Hy, Wx, p, pred_bstride);
    hipStream_t st = (hipStream_t)stream;
    const int xt = cdiv(Wx, TX), yt = cdiv(Hy, TY_), zt = cdiv(Lz, TZ);
    if (C == 4 && zt <= 65535 && B <= 65535 && ((uintptr_t)pred % 16 == 0) && pred_bstride % 4 == 0) {
        hipLaunchKernelGGL(loss_fwd_fused_kernel, dim3(xt * yt, zt, B), dim3(256), 0, st, pred, imgs, mask, edge_tgt, pred_vol,
                           edge_pred, acc, xt, g);
        return vitae_launch_status();
    }
    hipLaunchKernelGGL(recon_fwd_kernel, dim3(g.L, B), dim3(256), 0, st, pred, imgs, mask, acc, g);
    hipLaunchKernelGGL(unpatchify_kernel, dim3(g.L, B), dim3(256), 0, st, pred, pred_vol, g);
    return vitae_sobel_edge_fwd(pred_vol, edge_pred, edge_tgt, acc, B, C, Lz, Hy, Wx, stream);
}

extern "C" int vitae_loss_bwd_fused(const float* pred, const float* pred_vol, const float* imgs, const float* mask, const float* edge_pred,
                                    const float* edge_tgt, const float* hp, float* dG_ws, float* dpred, void* dpred_bf16,
                                    float* nonfinite_flag, long pred_bstride, float mask_sum, int B, int C, int Lz, int Hy,
                                    int Wx, int p, void* stream) {
    if (!pred || !pred_vol || !imgs || !mask || !edge_pred || !edge_tgt || !hp || !dpred || bad_extents(B, C, Lz, Hy, Wx) || B > 65535 ||
        bad_patches(Lz, Hy, Wx, p) || !(mask_sum > 0.f))
        return VITAE_ERR_INVALID_ARG;
    VolGeom g = make_geom(C, Lz, Hy, Wx, p, pred_bstride);
    const long total = (long)B * Lz * Hy * Wx;
    const float inv_count = 1.0f / (float)total, inv_pm = 1.0f / ((float)g.P * mask_sum);
    const int xt = cdiv(Wx, TX), yt = cdiv(Hy, TY_), zt = cdiv(Lz, TZ);
    hipStream_t st = (hipStream_t)stream;
    __bf16* d16 = reinterpret_cast<__bf16*>(dpred_bf16);
    const bool vec_ok = ((uintptr_t)dpred % 16 == 0) && ((uintptr_t)dpred_bf16 % 8 == 0) && pred_bstride % 4 == 0;
    if (zt <= 65535 && B <= 65535 && (C == 1 || (C == 4 && vec_ok))) {
        const bool row16 = Wx % 4 == 0 && ((uintptr_t)pred_vol % 16 == 0);
        const dim3 grid(xt * yt, zt, B);
#define VITAE_LBW(CH_, R_) hipLaunchKernelGGL((loss_bwd_fused_kernel<CH_, R_>), grid, dim3(256), 0, st, pred_vol, imgs, mask, edge_pred, \
                                              edge_tgt, hp, dpred, d16, nonfinite_flag, inv_count, inv_pm, xt, g)
        if (C == 1) { if (row16) VITAE_LBW(1, true); else VITAE_LBW(1, false); }
        else { if (row16) VITAE_LBW(4, true); else VITAE_LBW(4, false); }
#undef VITAE_LBW
        return vitae_launch_status();
    }
    // other channel counts: the three-kernel path (needs the dG scratch)
    if (!dG_ws) return VITAE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(recon_bwd_kernel, dim3(g.L, B), dim3(256), 0, st, pred, imgs, mask, hp, dpred, inv_pm, g);
    hipLaunchKernelGGL(sobel_bwd_components_kernel, dim3(stream_blocks(total)), dim3(256), 0, st, pred_vol, edge_pred,
                       edge_tgt, hp, dG_ws, inv_count, B, C, Lz, Hy, Wx);
    hipLaunchKernelGGL(sobel_bwd_scatter_kernel, dim3(stream_blocks(total)), dim3(256), 0, st, dG_ws, dpred, d16, B, g);
    return vitae_launch_status();
}

extern "C" int vitae_loss_finalize(const double* acc, const float* hp, float* out4, float mask_sum, long edge_count,
                                   void* stream) {
    if (!acc || !hp || !out4 || !(mask_sum > 0.f) || edge_count <= 0) return VITAE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, hp, out4, 1.0f / mask_sum,
                       1.0f / (float)edge_count);
    return vitae_launch_status();
}

extern "C" int vitae_cosine_loss_fwd(const float* p1, const float* z2, const float* p2, const float* z1, double* acc,
                                     const float* hp, float* out1, int R, int D, void* stream) {
    if (!p1 || !z2 || !p2 || !z1 || !acc || !hp || !out1 || R <= 0 || D <= 0) return VITAE_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    // (one row per wave up to 1024 workgroups: a wave that walks several rows is a chain of memory latencies — 26 us at 1732 rows on 256)
    const dim3 grid(cdiv(R, 4) < 1024 ? cdiv(R, 4) : 1024);
    const bool al = !(((uintptr_t)p1 | (uintptr_t)z2 | (uintptr_t)p2 | (uintptr_t)z1) & 15);
    if (al && (D == 768 || D == 1024 || D == 512 || D == 256)) {
        const float ir = 1.0f / (float)R;
        if (D == 768) hipLaunchKernelGGL(cosine_fwd_vec_kernel<3>, grid, dim3(256), 0, st, p1, z2, p2, z1, acc, hp, out1, ir, R, 1e-8f);
        else if (D == 1024) hipLaunchKernelGGL(cosine_fwd_vec_kernel<4>, grid, dim3(256), 0, st, p1, z2, p2, z1, acc, hp, out1, ir, R, 1e-8f);
        else if (D == 512) hipLaunchKernelGGL(cosine_fwd_vec_kernel<2>, grid, dim3(256), 0, st, p1, z2, p2, z1, acc, hp, out1, ir, R, 1e-8f);
        else hipLaunchKernelGGL(cosine_fwd_vec_kernel<1>, grid, dim3(256), 0, st, p1, z2, p2, z1, acc, hp, out1, ir, R, 1e-8f);
        return vitae_launch_status();
    }
    hipLaunchKernelGGL(cosine_fwd_kernel, dim3(cdiv(R, 4) < 1024 ? cdiv(R, 4) : 1024), dim3(256), 0, st, p1, z2, p2, z1, acc, R, D, 1e-8f);
    hipLaunchKernelGGL(cosine_finalize_kernel, dim3(1), dim3(64), 0, st, acc, hp, out1, 1.0f / (float)R);
    return vitae_launch_status();
}

extern "C" int vitae_cosine_loss_bwd(const float* p1, const float* z2, const float* p2, const float* z1,
                                     const float* hp, float* dp1, float* dp2, int R, int D, void* stream) {
    if (!p1 || !z2 || !p2 || !z1 || !hp || !dp1 || !dp2 || R <= 0 || D <= 0) return VITAE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cosine_bwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, p1, z2, p2, z1, hp, dp1,
                       dp2, (__bf16*)nullptr, (__bf16*)nullptr, R, D, 1e-8f);
    return vitae_launch_status();
}

// the same with bf16 copies of the gradients (what the predictor's LDS-DMA GEMMs consume); dp1 / dp2 may be NULL then
extern "C" int vitae_cosine_loss_bwd_bf16(const float* p1, const float* z2, const float* p2, const float* z1, const float* hp, float* dp1,
                                          float* dp2, void* dp1_bf16, void* dp2_bf16, int R, int D, void* stream) {
    if (!p1 || !z2 || !p2 || !z1 || !hp || !dp1_bf16 || !dp2_bf16 || (!dp1) != (!dp2) || R <= 0 || D <= 0) return VITAE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(cosine_bwd_kernel, dim3(cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, p1, z2, p2, z1, hp, dp1, dp2,
                       reinterpret_cast<__bf16*>(dp1_bf16), reinterpret_cast<__bf16*>(dp2_bf16), R, D, 1e-8f);
    return vitae_launch_status();
}
