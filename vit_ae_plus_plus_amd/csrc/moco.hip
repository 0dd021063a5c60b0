// MoCo v3 around the encoder (ABI 55; bf16 weight shadows: ABI 57): the momentum update, LARS and the InfoNCE loss of other_baselines/mocov3/moco as
// launches over whole parameter lists / whole batches.  All memory- or latency-bound: wave reductions, no MFMA.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "vitae_hip.h"
#include "common.hpp"

// This file is built with -ffp-contract=off (build.py EXTRA_FLAGS), unlike the rest of the library: every product is rounded before it
// is added.  The momentum update is specified as two products and one sum, and LARS forms g + wd p twice (norm pass, update pass) and
// must get the same value.

namespace {

struct MultiEntry { float* p; const float* g; float* m; long long flags; long long n; long long group; };
static_assert(sizeof(MultiEntry) == 8 * VITAE_MULTI_ENTRY_WORDS, "table entry layout (vitae_hip.h)");

// sum of two doubles over the 256 threads of a workgroup, in a fixed order; every thread gets the result
__device__ __forceinline__ void block_sum2_f64(double& a, double& b, double (*red)[2]) {
#pragma unroll
    for (int d = 32; d; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    __syncthreads();                      // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = a; red[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    a = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    b = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
}

// ---- bf16 shadows (ABI 57): the update that stores a new fp32 weight also stores its bf16 copy, with cast_bf16_kernel's conversion
// (gemm_bf16.hip), so the encoders' GEMMs need no cast launch afterwards.  SH is a compile-time flag: without it the bodies below are
// the kernels of ABI 55, instruction for instruction.  shadow[t]: device address of tensor t's bf16 copy, 0 = none.
template <bool SH>
__device__ __forceinline__ __bf16* shadow_of(const long long* shadow, int t, long off) {
    if constexpr (SH) {
        const long long a = shadow[t];
        return a ? reinterpret_cast<__bf16*>(a) + off : nullptr;
    }
    return nullptr;
}
__device__ __forceinline__ void shadow_store4(__bf16* sh, long i, const f32x4 v) {
    bf16x4 h;
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] = (__bf16)v[k];
    reinterpret_cast<bf16x4*>(sh)[i] = h;             // one 8-byte store
}

// ---- momentum update: pm <- pm m + pb (1 - m)
template <int U, bool SH>
__device__ __forceinline__ void ema_multi_body(const MultiEntry* table, const int* chunks, long n_chunks,
                                               long chunk, float m, float omm, const long long* shadow) {
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int t = chunks[2 * c];
        const MultiEntry e = table[t];
        const long off = (long)chunks[2 * c + 1] * chunk;
        const long len = e.n - off < chunk ? e.n - off : chunk;
        float* pm = e.p + off;
        const float* pb = e.g + off;
        __bf16* sh = shadow_of<SH>(shadow, t, off);
        long done = 0;
        // chunk and off are multiples of 4: the chunk is 16-byte aligned exactly when the tensor's base addresses are (and its shadow
        // 8-byte aligned exactly when the shadow's base address is)
        if (!(((uintptr_t)pm | (uintptr_t)pb) & 15) && !((uintptr_t)sh & 7)) {
            const long n4 = len / 4;
            f32x4* pm4 = reinterpret_cast<f32x4*>(pm);
            const f32x4* pb4 = reinterpret_cast<const f32x4*>(pb);
            for (long i0 = threadIdx.x; i0 < n4; i0 += U * 256) {
                f32x4 a[U], b[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const long i = i0 + u * 256 < n4 ? i0 + u * 256 : i0;
                    a[u] = pm4[i];
                    b[u] = __builtin_nontemporal_load(pb4 + i);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (i0 + u * 256 >= n4) break;
                    const f32x4 r = a[u] * m + b[u] * omm;
                    pm4[i0 + u * 256] = r;
                    if (SH && sh) shadow_store4(sh, i0 + u * 256, r);
                }
            }
            done = n4 * 4;
        }
        for (long i = done + threadIdx.x; i < len; i += 256) {
            const float r = pm[i] * m + pb[i] * omm;
            pm[i] = r;
            if (SH && sh) sh[i] = (__bf16)r;
        }
    }
}

template <int U>
__global__ __launch_bounds__(256) void ema_multi_kernel(const MultiEntry* __restrict__ table, const int* __restrict__ chunks, long n_chunks,
                                                        long chunk, float m, float omm) {
    ema_multi_body<U, false>(table, chunks, n_chunks, chunk, m, omm, nullptr);
}

template <int U>
__global__ __launch_bounds__(256) void ema_multi_shadow_kernel(const MultiEntry* __restrict__ table, const int* __restrict__ chunks,
                                                               long n_chunks, long chunk, float m, float omm,
                                                               const long long* __restrict__ shadow) {
    ema_multi_body<U, true>(table, chunks, n_chunks, chunk, m, omm, shadow);
}

// ---- LARS, launch 1: per chunk of a scaled tensor, sum p^2 and sum (g + wd p)^2 in double
__global__ __launch_bounds__(256) void lars_norm_kernel(const MultiEntry* __restrict__ table, const int* __restrict__ chunks, long n_chunks,
                                                        long chunk, const float* __restrict__ hp, int n_groups, double* __restrict__ ws) {
    __shared__ double red[4][2];
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const MultiEntry e = table[chunks[2 * c]];
        if (!(e.flags & VITAE_LARS_FLAG_SCALED)) continue;           // (uniform over the workgroup)
        const long off = (long)chunks[2 * c + 1] * chunk;
        const long len = e.n - off < chunk ? e.n - off : chunk;
        const float wd = hp[n_groups + e.group];
        const float* p = e.p + off;
        const float* g = e.g + off;
        double sp = 0.0, sd = 0.0;
        long done = 0;
        if (!(((uintptr_t)p | (uintptr_t)g) & 15)) {
            const long n4 = len / 4;
            for (long i = threadIdx.x; i < n4; i += 256) {
                const f32x4 pv = reinterpret_cast<const f32x4*>(p)[i], gv = reinterpret_cast<const f32x4*>(g)[i];
                const f32x4 dv = gv + pv * wd;
#pragma unroll
                for (int k = 0; k < 4; ++k) { sp += (double)pv[k] * (double)pv[k]; sd += (double)dv[k] * (double)dv[k]; }
            }
            done = n4 * 4;
        }
        for (long i = done + threadIdx.x; i < len; i += 256) {
            const float pe = p[i], de = g[i] + pe * wd;
            sp += (double)pe * (double)pe; sd += (double)de * (double)de;
        }
        block_sum2_f64(sp, sd, red);
        if (threadIdx.x == 0) { ws[2 * c] = sp; ws[2 * c + 1] = sd; }
    }
}

// ---- LARS, launch 2: the trust ratio of the chunk's tensor from the partials (in chunk order), then the update
template <int U, bool SH>
__device__ __forceinline__ void lars_step_body(const MultiEntry* table, const int* chunks, long n_chunks,
                                               long chunk, const float* hp, int n_groups, const double* ws,
                                               const long long* shadow) {
    __shared__ double red[4][2];
    int cur_t = -1;
    float q = 1.f;
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int t = chunks[2 * c], k = chunks[2 * c + 1];
        const MultiEntry e = table[t];
        const bool scaled = e.flags & VITAE_LARS_FLAG_SCALED;
        if (scaled && t != cur_t) {                                   // (uniform over the workgroup)
            const long first = c - k, count = (e.n + chunk - 1) / chunk;
            double sp = 0.0, sd = 0.0;
            for (long j = threadIdx.x; j < count; j += 256) { sp += ws[2 * (first + j)]; sd += ws[2 * (first + j) + 1]; }
            block_sum2_f64(sp, sd, red);
            const double trust = (double)hp[3 * n_groups + e.group];
            q = (sp > 0.0 && sd > 0.0) ? (float)(trust * sqrt(sp) / sqrt(sd)) : 1.f;
            cur_t = t;
        }
        const float lr = hp[e.group], wd = hp[n_groups + e.group], mom = hp[2 * n_groups + e.group];
        const long off = (long)k * chunk;
        const long len = e.n - off < chunk ? e.n - off : chunk;
        float* p = e.p + off;
        const float* g = e.g + off;
        float* mu = e.m + off;
        __bf16* sh = shadow_of<SH>(shadow, t, off);
        long done = 0;
        if (!(((uintptr_t)p | (uintptr_t)g | (uintptr_t)mu) & 15) && !((uintptr_t)sh & 7)) {
            const long n4 = len / 4;
            f32x4* p4 = reinterpret_cast<f32x4*>(p);
            f32x4* m4 = reinterpret_cast<f32x4*>(mu);
            const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
            for (long i0 = threadIdx.x; i0 < n4; i0 += U * 256) {
                f32x4 pv[U], mv[U], gv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const long i = i0 + u * 256 < n4 ? i0 + u * 256 : i0;
                    pv[u] = p4[i]; mv[u] = m4[i]; gv[u] = __builtin_nontemporal_load(g4 + i);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (i0 + u * 256 >= n4) break;
                    const f32x4 dp = scaled ? (gv[u] + pv[u] * wd) * q : gv[u];
                    const f32x4 mn = mv[u] * mom + dp;
                    m4[i0 + u * 256] = mn;
                    const f32x4 pn = pv[u] - mn * lr;
                    p4[i0 + u * 256] = pn;
                    if (SH && sh) shadow_store4(sh, i0 + u * 256, pn);
                }
            }
            done = n4 * 4;
        }
        for (long i = done + threadIdx.x; i < len; i += 256) {
            const float pe = p[i];
            const float dp = scaled ? (g[i] + pe * wd) * q : g[i];
            const float mn = mu[i] * mom + dp;
            mu[i] = mn;
            const float pn = pe - mn * lr;
            p[i] = pn;
            if (SH && sh) sh[i] = (__bf16)pn;
        }
    }
}

template <int U>
__global__ __launch_bounds__(256) void lars_step_kernel(const MultiEntry* __restrict__ table, const int* __restrict__ chunks, long n_chunks,
                                                        long chunk, const float* __restrict__ hp, int n_groups, const double* __restrict__ ws) {
    lars_step_body<U, false>(table, chunks, n_chunks, chunk, hp, n_groups, ws, nullptr);
}

template <int U>
__global__ __launch_bounds__(256) void lars_step_shadow_kernel(const MultiEntry* __restrict__ table, const int* __restrict__ chunks,
                                                               long n_chunks, long chunk, const float* __restrict__ hp, int n_groups,
                                                               const double* __restrict__ ws, const long long* __restrict__ shadow) {
    lars_step_body<U, true>(table, chunks, n_chunks, chunk, hp, n_groups, ws, shadow);
}

// ---- InfoNCE.  ws: double rowloss[2 N] | double denom[4 N] (max(|x|, 1e-12) of the rows of q1, k2, q2, k1)
// Everything between the fp32 inputs and the fp32 outputs is double: the rows are short and few, and what the float64 reference is
// compared with is then the rounding of the results, not of a chain of fp32 intermediates (normalised rows, logits up to 1 / T).
__global__ __launch_bounds__(256) void moco_norm_kernel(const float* __restrict__ q1, const float* __restrict__ k2, const float* __restrict__ q2,
                                                        const float* __restrict__ k1, int N, int C, double* __restrict__ denom) {
    __shared__ double red[4][2];
    const int which = blockIdx.x / N, r = blockIdx.x % N;
    const float* x = (which == 0 ? q1 : which == 1 ? k2 : which == 2 ? q2 : k1) + (long)r * C;
    double s = 0.0, unused = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) s += (double)x[c] * (double)x[c];
    block_sum2_f64(s, unused, red);
    const double nrm = sqrt(s);
    if (threadIdx.x == 0) denom[blockIdx.x] = nrm > 1e-12 ? nrm : 1e-12;          // F.normalize: x / max(|x|, eps)
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void moco_row_kernel(const float* __restrict__ q1, const float* __restrict__ k2, const float* __restrict__ q2,
                                                       const float* __restrict__ k1, const double* __restrict__ denom, int N, int C, double T,
                                                       double* __restrict__ rowloss, float* __restrict__ dq1, float* __restrict__ dq2) {
    __shared__ double lg[VITAE_MOCO_MAX_N];           // logits, then the coefficients of the key rows in dqn
    __shared__ double dqn[VITAE_MOCO_MAX_C];          // gradient with respect to the normalised query row
    __shared__ double red[4][2];
    const int pair = blockIdx.x / N, i = blockIdx.x % N;
    const float* q = (pair == 0 ? q1 : q2) + (long)i * C;
    const float* k = pair == 0 ? k2 : k1;
    const double dq_ = denom[(2 * pair) * N + i];
    const double* dk = denom + (2 * pair + 1) * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < N; j += 4) {
        const float* kr = k + (long)j * C;
        double a = 0.0;
        for (int c = lane; c < C; c += 64) a += (double)q[c] * (double)kr[c];
        a = wave_sum_f64(a);
        if (lane == 0) lg[j] = a / (dq_ * dk[j]) / T;
    }
    __syncthreads();
    double mx = -INFINITY, unused = 0.0;
    for (int j = 0; j < N; ++j) mx = fmax(mx, lg[j]);           // (every thread, the same order: LDS broadcasts)
    double s = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) s += exp(lg[j] - mx);
    block_sum2_f64(s, unused, red);
    const double self = lg[i];
    if (threadIdx.x == 0) rowloss[blockIdx.x] = log(s) + (mx - self);
    __syncthreads();                                      // every thread has read lg[i]
    // d loss / d logit_j = (2 T / N) (softmax_j - [j == i]); through the division by T and the key's normalisation: (2 / N) (...) / |k_j|
    for (int j = threadIdx.x; j < N; j += 256) lg[j] = (exp(lg[j] - mx) / s - (j == i ? 1.0 : 0.0)) * (2.0 / (double)N) / dk[j];
    __syncthreads();
    double dot = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        double a = 0.0;
        for (int j = 0; j < N; ++j) a += lg[j] * (double)k[(long)j * C + c];
        dqn[c] = a;                                       // (read back below by the thread that wrote it)
        dot += a * ((double)q[c] / dq_);
    }
    block_sum2_f64(dot, unused, red);
    // the clamped norm is a constant: no projection term for such a row
    const double proj = dq_ > 1e-12 ? dot : 0.0;
    float* dq = (pair == 0 ? dq1 : dq2) + (long)i * C;
    for (int c = threadIdx.x; c < C; c += 256) dq[c] = (float)((dqn[c] - ((double)q[c] / dq_) * proj) / dq_);
}

__global__ __launch_bounds__(256) void moco_loss_sum_kernel(const double* __restrict__ rowloss, int N, double T, float* __restrict__ loss) {
    __shared__ double red[4][2];
    double s = 0.0, unused = 0.0;
    for (int r = threadIdx.x; r < 2 * N; r += 256) s += rowloss[r];
    block_sum2_f64(s, unused, red);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)N * (2.0 * T));
}

// the whole call is judged on the host copies before the first launch
int multi_check(const long long* table, long n_entries, const int* chunks, long n_chunks, long chunk, int n_groups, bool lars) {
    if (n_entries < 0 || n_chunks < 0 || chunk <= 0 || (chunk & 3)) return VITAE_ERR_INVALID_ARG;
    if (n_entries == 0 || n_chunks == 0) return VITAE_OK;
    if (!table || !chunks) return VITAE_ERR_INVALID_ARG;
    for (long t = 0; t < n_entries; ++t) {
        const long long* e = table + t * VITAE_MULTI_ENTRY_WORDS;
        if (!e[0] || !e[1] || e[4] < 0) return VITAE_ERR_INVALID_ARG;
        if (lars && (!e[2] || e[5] < 0 || e[5] >= n_groups)) return VITAE_ERR_INVALID_ARG;
    }
    long pt = -1, pk = -1;
    for (long c = 0; c < n_chunks; ++c) {
        const long t = chunks[2 * c], k = chunks[2 * c + 1];
        if (t < 0 || t >= n_entries || k < 0 || (long long)k * chunk >= table[t * VITAE_MULTI_ENTRY_WORDS + 4]) return VITAE_ERR_INVALID_ARG;
        if (lars) {     // tensor order, the chunks of a tensor ascending and complete: launch 2 finds a tensor's partials at c - k
            const bool same = t == pt && k == pk + 1, next = t > pt && k == 0;
            if (!same && !next) return VITAE_ERR_INVALID_ARG;
            if (next && pt >= 0 && (pk + 1) * chunk < table[pt * VITAE_MULTI_ENTRY_WORDS + 4]) return VITAE_ERR_INVALID_ARG;
            pt = t; pk = k;
        }
    }
    if (lars && (pk + 1) * chunk < table[pt * VITAE_MULTI_ENTRY_WORDS + 4]) return VITAE_ERR_INVALID_ARG;
    return VITAE_OK;
}

// the shadow column of a *_shadow call, judged on its host copy like the table: every address even (a bf16 address)
int shadow_check(const long long* shadow_host, long n_entries) {
    for (long t = 0; t < n_entries; ++t)
        if (shadow_host[t] & 1) return VITAE_ERR_INVALID_ARG;
    return VITAE_OK;
}

}  // namespace

extern "C" int vitae_ema_multi(const long long* table_host, const long long* table_dev, long n_entries, const int* chunks_host,
                               const int* chunks_dev, long n_chunks, long chunk, double m, void* stream) {
    if (!(m >= 0.0 && m <= 1.0)) return VITAE_ERR_INVALID_ARG;
    const int rc = multi_check(table_host, n_entries, chunks_host, n_chunks, chunk, 0, false);
    if (rc != VITAE_OK || n_entries == 0 || n_chunks == 0) return rc;
    if (!table_dev || !chunks_dev) return VITAE_ERR_INVALID_ARG;
    // 12 bytes per element and nothing to compute: two workgroups per CU keep the loads in flight
    const long blocks = n_chunks < 512 ? n_chunks : 512;
    hipLaunchKernelGGL(ema_multi_kernel<4>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const MultiEntry*>(table_dev), chunks_dev, n_chunks, chunk, (float)m, (float)(1. - m));
    return vitae_launch_status();
}

extern "C" int vitae_ema_multi_shadow(const long long* table_host, const long long* table_dev, long n_entries, const int* chunks_host,
                                      const int* chunks_dev, long n_chunks, long chunk, double m, const long long* shadow_host,
                                      const long long* shadow_dev, void* stream) {
    if (!shadow_host && !shadow_dev) return vitae_ema_multi(table_host, table_dev, n_entries, chunks_host, chunks_dev, n_chunks, chunk, m, stream);
    if (!shadow_host || !shadow_dev) return VITAE_ERR_INVALID_ARG;
    if (!(m >= 0.0 && m <= 1.0)) return VITAE_ERR_INVALID_ARG;
    const int rc = multi_check(table_host, n_entries, chunks_host, n_chunks, chunk, 0, false);
    if (rc != VITAE_OK || n_entries == 0 || n_chunks == 0) return rc;
    if (!table_dev || !chunks_dev || shadow_check(shadow_host, n_entries) != VITAE_OK) return VITAE_ERR_INVALID_ARG;
    // vitae_ema_multi's grid: 14 bytes per element where a shadow is listed
    const long blocks = n_chunks < 512 ? n_chunks : 512;
    hipLaunchKernelGGL(ema_multi_shadow_kernel<4>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const MultiEntry*>(table_dev), chunks_dev, n_chunks, chunk, (float)m, (float)(1. - m), shadow_dev);
    return vitae_launch_status();
}

extern "C" int vitae_lars_multi(const long long* table_host, const long long* table_dev, long n_entries, const int* chunks_host,
                                const int* chunks_dev, long n_chunks, long chunk, const float* group_hp_dev, int n_groups, double* ws,
                                void* stream) {
    if (n_groups < 1 || n_groups > VITAE_MULTI_MAX_GROUPS || !group_hp_dev) return VITAE_ERR_INVALID_ARG;
    const int rc = multi_check(table_host, n_entries, chunks_host, n_chunks, chunk, n_groups, true);
    if (rc != VITAE_OK || n_entries == 0 || n_chunks == 0) return rc;
    if (!table_dev || !chunks_dev || !ws || ((uintptr_t)ws & 7)) return VITAE_ERR_INVALID_ARG;
    const MultiEntry* table = reinterpret_cast<const MultiEntry*>(table_dev);
    // The norm pass only reads: up to four workgroups per CU, as vitae_grad_sqnorm_multi.  The update pass has vitae_adamw_multi's access
    // pattern (p, g and state read, p and state written, four 16-byte groups in flight per thread) and takes its grid, one workgroup
    // per CU, which was swept there (LABNOTES, multi-tensor AdamW); it was not swept again here, where it moves its 20 B per parameter
    // of ViT-B's 121 M in 0.65 ms together with the norm pass.
    const long nb = n_chunks < 1024 ? n_chunks : 1024, sb = n_chunks < 256 ? n_chunks : 256;
    hipLaunchKernelGGL(lars_norm_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, table, chunks_dev, n_chunks, chunk, group_hp_dev,
                       n_groups, ws);
    hipLaunchKernelGGL(lars_step_kernel<4>, dim3((int)sb), dim3(256), 0, (hipStream_t)stream, table, chunks_dev, n_chunks, chunk,
                       group_hp_dev, n_groups, ws);
    return vitae_launch_status();
}

extern "C" int vitae_lars_multi_shadow(const long long* table_host, const long long* table_dev, long n_entries, const int* chunks_host,
                                       const int* chunks_dev, long n_chunks, long chunk, const float* group_hp_dev, int n_groups, double* ws,
                                       const long long* shadow_host, const long long* shadow_dev, void* stream) {
    if (!shadow_host && !shadow_dev)
        return vitae_lars_multi(table_host, table_dev, n_entries, chunks_host, chunks_dev, n_chunks, chunk, group_hp_dev, n_groups, ws, stream);
    if (!shadow_host || !shadow_dev) return VITAE_ERR_INVALID_ARG;
    if (n_groups < 1 || n_groups > VITAE_MULTI_MAX_GROUPS || !group_hp_dev) return VITAE_ERR_INVALID_ARG;
    const int rc = multi_check(table_host, n_entries, chunks_host, n_chunks, chunk, n_groups, true);
    if (rc != VITAE_OK || n_entries == 0 || n_chunks == 0) return rc;
    if (!table_dev || !chunks_dev || !ws || ((uintptr_t)ws & 7)) return VITAE_ERR_INVALID_ARG;
    if (shadow_check(shadow_host, n_entries) != VITAE_OK) return VITAE_ERR_INVALID_ARG;
    const MultiEntry* table = reinterpret_cast<const MultiEntry*>(table_dev);
    // vitae_lars_multi's two launches and grids; only the second one writes, and only it knows the shadows (22 bytes per element there)
    const long nb = n_chunks < 1024 ? n_chunks : 1024, sb = n_chunks < 256 ? n_chunks : 256;
    hipLaunchKernelGGL(lars_norm_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, table, chunks_dev, n_chunks, chunk, group_hp_dev,
                       n_groups, ws);
    hipLaunchKernelGGL(lars_step_shadow_kernel<4>, dim3((int)sb), dim3(256), 0, (hipStream_t)stream, table, chunks_dev, n_chunks, chunk,
                       group_hp_dev, n_groups, ws, shadow_dev);
    return vitae_launch_status();
}

extern "C" long vitae_moco_loss_ws_floats(int N, int C) {
    if (N < 1 || C < 1) return 0;
    return 12L * N;                 // 6 N doubles
}

extern "C" int vitae_moco_loss(const float* q1, const float* k2, const float* q2, const float* k1, int N, int C, double T, float* loss,
                               float* dq1, float* dq2, float* ws, void* stream) {
    if (!q1 || !k2 || !q2 || !k1 || !loss || !dq1 || !dq2 || !ws || ((uintptr_t)ws & 15) || N < 1 || C < 1) return VITAE_ERR_INVALID_ARG;
    if (!(T > 0.0) || !isfinite(T)) return VITAE_ERR_INVALID_ARG;
    if (N > VITAE_MOCO_MAX_N || C > VITAE_MOCO_MAX_C) return VITAE_ERR_UNSUPPORTED_SHAPE;
    double* rowloss = reinterpret_cast<double*>(ws);
    double* denom = rowloss + 2L * N;
    hipLaunchKernelGGL(moco_norm_kernel, dim3(4 * N), dim3(256), 0, (hipStream_t)stream, q1, k2, q2, k1, N, C, denom);
    hipLaunchKernelGGL(moco_row_kernel, dim3(2 * N), dim3(256), 0, (hipStream_t)stream, q1, k2, q2, k1, denom, N, C, T, rowloss, dq1, dq2);
    hipLaunchKernelGGL(moco_loss_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rowloss, N, T, loss);
    return vitae_launch_status();
}
