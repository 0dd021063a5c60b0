// Optimiser-side streaming kernels over the flat parameter / gradient arenas (HBM-bound):
//   global gradient L2 norm     utils/misc.py:265-266, 280-292  (reference op K25)
//   AdamW step                  torch.optim.AdamW(betas=(0.9, 0.95)) created at
//                               k_fold_training_scripts/k_fold_cross_valid_combined_brats.py:168-169 (op K26)
// Hyper-parameters live in the device `hp` block (VITAE_HP_*), so a captured step graph can be
// replayed while lr / bias corrections change.  The step is skipped when the gradient norm is not
// finite — the effect of GradScaler.step's inf check (utils/misc.py:267).
#include <cstdlib>
#include "common.hpp"
#include "vitae_hip.h"

namespace {

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// Gradients are read either as fp32 or as bf16 (the wire copy of a data-parallel all-reduce done in bf16: the
// optimiser then consumes the reduced values directly instead of a converted fp32 copy).
template <typename G> __device__ __forceinline__ f32x4 grad4(const G* g, long i);
template <> __device__ __forceinline__ f32x4 grad4<float>(const float* g, long i) {
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
}
template <> __device__ __forceinline__ f32x4 grad4<__bf16>(const __bf16* g, long i) {
    const bf16x4 h = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(g) + i);
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// where workgroup b adds its share of the squared gradient norm: spread slots (same-address double atomics retire one per ~10 ns)
__device__ __forceinline__ double* gradsq_slot(double* acc) {
    return acc + VITAE_ACC_SQ_BASE + ((int)blockIdx.x & (VITAE_ACC_SQ_SLOTS - 1)) * VITAE_ACC_SQ_STRIDE;
}

template <typename G>
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const G* __restrict__ g, long n, double* __restrict__ acc) {
    __shared__ float red[4];
    float s = 0.f;
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = grad4<G>(g, i);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0) for (long i = n4 * 4 + threadIdx.x; i < n; i += 256) s += (float)g[i] * (float)g[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) atomicAdd(gradsq_slot(acc), (double)s);
}

// one wave: lane s reads spread slot s (vitae_hip.h VITAE_ACC_SQ_*), lane 0 adds acc[GRADSQ]
__global__ __launch_bounds__(64) void grad_norm_finalize_kernel(const double* __restrict__ acc, float* __restrict__ out) {
    static_assert(VITAE_ACC_SQ_SLOTS == 64, "one slot per lane");
    double v = acc[VITAE_ACC_SQ_BASE + threadIdx.x * VITAE_ACC_SQ_STRIDE];
    if (threadIdx.x == 0) v += acc[VITAE_ACC_GRADSQ];
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (float)sqrt(v);
}

// 1 - beta^t on the device.  A NEGATIVE slot carries -(1 - beta) from the host's double (relative error 6e-8; fp32(0.999) itself is
// 1.3e-8 off, which is 1.3e-5 of 1 - 0.999^t for small t): 1 - beta^t = -expm1(t log1p(-(1 - beta))).  Slot == 0: from fp32 beta.
__device__ __forceinline__ void device_bias_corrections(float omb1, float omb2, float t, float& bc1, float& bc2) {
    // the products are rounded HERE in every instantiation: the empty asm keeps them out of a fused multiply-add at the top of expm1f
    float x1 = t * log1pf(-omb1), x2 = t * log1pf(-omb2);
    asm volatile("" : "+v"(x1), "+v"(x2));
    bc1 = -expm1f(x1);
    bc2 = -expm1f(x2);
}

// 1 - beta as the moment updates and the bias corrections use it: the host's double-formed value when the slot carries it (negative
// slot), else 1.f - fp32(beta).  The latter is 4.7e-5 off 1 - 0.999 (fp32(0.999) is 1.3e-8 off, all of which lands in the difference)
// and so is every (1 - beta2) g^2 formed from it: 2.4-6.4 times the error of a plain fp32 AdamW at beta2 = 0.999, none at 0.95.
__device__ __forceinline__ float one_minus_beta(float slot, float b) { return slot < 0.f ? -slot : 1.f - b; }

// One element of the step with every fused multiply-add spelled out.  The library is built with -ffp-contract=fast, and where a sum has
// two products (b2 v + (1 - b2) g^2; g gs - m; 1 - lr wd) the compiler is free to fuse either one.  In the scalar tail of adamw_kernel it
// chose differently for fp32 and for bf16 gradients: v of a tail element differed in the last bit between vitae_adamw_step and
// vitae_adamw_step_bf16g on the same values once v was not zero (tests/test_optimizer_kernels.py).  Written this way the gradient and
// moment types, the unrolled groups, the scalar tail and vitae_opt_tail all round alike, and GRAD_MUL = 2^-k on gradients x 2^k is exact.
__device__ __forceinline__ float adamw_decay(float lr, float weight_decay) { return __builtin_fmaf(-lr, weight_decay, 1.0f); }
__device__ __forceinline__ void adamw_element(float& p, float& m, float& v, float g, float gs, float decay, float omb1, float b2, float omb2,
                                              float step, float sq_bc2, float eps) {
    m = __builtin_fmaf(omb1, __builtin_fmaf(g, gs, -m), m);              // exp_avg.lerp_(grad, 1 - beta1)
    const float ge = g * gs;
    v = __builtin_fmaf(b2, v, omb2 * ge * ge);
    p = __builtin_fmaf(-step, m / (sqrtf(v) / sq_bc2 + eps), p * decay);
}

// The moments are stored either as fp32 or as bf16 (round 6: `S`).  bf16 moments: the step is COMPUTED in fp32 from the stored
// values — m_new and v_new enter the parameter update unrounded — and only what is written back for the next step is rounded, so the
// stored moment carries a relative error of 2^-9 per step that decays with beta (tools/opt_state_ablation.py: the pinned ViT-B
// trajectory moves by 2e-7..2e-6, an 80-step loss curve by 1e-7, where another masking seed moves it by 1e-3).  8 B per parameter
// less HBM traffic (30 -> 22).  Round-to-nearest would stall an update smaller than half an ulp: the launchers refuse 1 - beta < 2^-6.
template <typename S> __device__ __forceinline__ f32x4 state4_ld(const S* s, long i);
template <> __device__ __forceinline__ f32x4 state4_ld<float>(const float* s, long i) {
    return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(s) + i);
}
template <> __device__ __forceinline__ f32x4 state4_ld<__bf16>(const __bf16* s, long i) {
    const bf16x4 h = __builtin_nontemporal_load(reinterpret_cast<const bf16x4*>(s) + i);
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
template <typename S> __device__ __forceinline__ void state4_st(S* s, long i, const f32x4 v);
template <> __device__ __forceinline__ void state4_st<float>(float* s, long i, const f32x4 v) {
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(s) + i);
}
template <> __device__ __forceinline__ void state4_st<__bf16>(__bf16* s, long i, const f32x4 v) {
    bf16x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) h[e] = (__bf16)v[e];
    __builtin_nontemporal_store(h, reinterpret_cast<bf16x4*>(s) + i);
}

// torch.optim.AdamW (single-tensor form): p *= 1 - lr*wd; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p -= (lr / bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
template <bool NT, typename G, int U = 8, typename S = float>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const G* __restrict__ g, S* __restrict__ m,
                                                    S* __restrict__ v, __bf16* __restrict__ shadow, long n,
                                                    const float* __restrict__ hp, const float* __restrict__ gnorm,
                                                    float weight_decay, const double* __restrict__ gacc = nullptr) {
    if (gnorm) { const float gn = gnorm[0]; if (!(gn == gn) || fabsf(gn) == INFINITY) return; }
    if (gacc) {
        // the gate straight from the accumulator (round 6): what grad_norm_finalize_kernel would have written for this bucket — every
        // wave sums the 64 spread slots + acc[GRADSQ] itself (65 L2 hits) instead of one more 4-5 us node in front of every bucket
        double q = gacc[VITAE_ACC_SQ_BASE + (threadIdx.x & 63) * VITAE_ACC_SQ_STRIDE];
        if ((threadIdx.x & 63) == 0) q += gacc[VITAE_ACC_GRADSQ];
#pragma unroll
        for (int d = 32; d; d >>= 1) q += __shfl_xor(q, d, 64);
        const float gn = (float)sqrt(q);
        if (!(gn == gn) || fabsf(gn) == INFINITY) return;
    }
    const float lr = hp[VITAE_HP_LR], b1 = hp[VITAE_HP_BETA1], b2 = hp[VITAE_HP_BETA2], eps = hp[VITAE_HP_EPS];
    float bc1 = hp[VITAE_HP_BC1], bc2 = hp[VITAE_HP_BC2];
    const float omb1 = one_minus_beta(bc1, b1), omb2 = one_minus_beta(bc2, b2);
    if (bc1 <= 0.f) {            // the host left the bias corrections to the device: t = applied steps + 1 (vitae_hip.h VITAE_HP_STEP)
        const float t = hp[VITAE_HP_STEP] + 1.f;
        device_bias_corrections(omb1, omb2, t, bc1, bc2);
    }
    const float sq_bc2 = sqrtf(bc2);
    const float gs = hp[VITAE_HP_GRAD_MUL];
    const float decay = adamw_decay(lr, weight_decay), step = lr / bc1;
    const long n4 = n / 4;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    // two independent 16-byte groups per thread and iteration: 8 loads in flight before the first dependent use.
    // The moments stream through (nothing re-reads them for a whole step): non-temporal loads and stores keep them
    // from evicting the bf16 shadow / activations out of L2 and the MALL.
    // U independent 16-byte groups per thread and iteration (4 U loads in flight before the first dependent use): the pass
    // runs on one workgroup per CU, so its rate is set by the bytes each wave keeps in flight
    const long stride = (long)gridDim.x * 256;
    for (long i0 = (long)blockIdx.x * 256 + threadIdx.x; i0 < n4; i0 += U * stride) {
        long idx[U];
        bool live[U];
        f32x4 pp[U], mm[U], vv[U], gg[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            live[u] = i0 + u * stride < n4;
            idx[u] = live[u] ? i0 + u * stride : i0;
            pp[u] = p4[idx[u]];
            mm[u] = state4_ld<S>(m, idx[u]);
            vv[u] = state4_ld<S>(v, idx[u]);
            gg[u] = grad4<G>(g, idx[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!live[u]) break;
            const long i = idx[u];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pp[u][e], me = mm[u][e], ve = vv[u][e];
                adamw_element(pe, me, ve, gg[u][e], gs, decay, omb1, b2, omb2, step, sq_bc2, eps);
                pp[u][e] = pe; mm[u][e] = me; vv[u][e] = ve;
            }
            p4[i] = pp[u];
            state4_st<S>(m, i, mm[u]);
            state4_st<S>(v, i, vv[u]);
            if (shadow) {
                bf16x4 sh;
#pragma unroll
                for (int e = 0; e < 4; ++e) sh[e] = (__bf16)pp[u][e];
                reinterpret_cast<bf16x4*>(shadow)[i] = sh;
            }
        }
    }
    if (blockIdx.x == 0) {
        for (long i = n4 * 4 + threadIdx.x; i < n; i += 256) {
            float pp = p[i], mm = (float)m[i], vv = (float)v[i];
            adamw_element(pp, mm, vv, (float)g[i], gs, decay, omb1, b2, omb2, step, sq_bc2, eps);
            p[i] = pp; m[i] = (S)mm; v[i] = (S)vv;
            if (shadow) shadow[i] = (__bf16)pp;
        }
    }
}

__global__ void opt_count_bump_kernel(float* __restrict__ hp, const float* __restrict__ gnorm) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float gn = gnorm ? gnorm[0] : 0.f;
        if (gn == gn && fabsf(gn) != INFINITY) hp[VITAE_HP_STEP] += 1.f;
    }
}

// ---- the tail of a step: tokens + vectors (0.2 M elements) in two launches
template <typename G>
__global__ __launch_bounds__(256) void opt_tail_norm_kernel(const G* __restrict__ g, long n, double* __restrict__ acc, float* __restrict__ out) {
    __shared__ float red[4];
    __shared__ int last;
    float s = 0.f;
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = grad4<G>(g, i);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    if (blockIdx.x == 0) for (long i = n4 * 4 + threadIdx.x; i < n; i += 256) s += (float)g[i] * (float)g[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) {
        atomicAdd(gradsq_slot(acc), (double)s);
        __threadfence();
        last = atomicAdd(reinterpret_cast<int*>(acc + VITAE_ACC_TICKET_A), 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (last && threadIdx.x < 64) {
        // every other workgroup's double atomic is ordered before its ticket: read the slots through the atomic unit too
        double tot = atomicAdd(acc + VITAE_ACC_SQ_BASE + threadIdx.x * VITAE_ACC_SQ_STRIDE, 0.0);
        if (threadIdx.x == 0) tot += atomicAdd(acc + VITAE_ACC_GRADSQ, 0.0);
#pragma unroll
        for (int d = 32; d; d >>= 1) tot += __shfl_xor(tot, d, 64);
        if (threadIdx.x == 0) out[0] = (float)sqrt(tot);
    }
}

template <typename G, typename S = float>
__global__ __launch_bounds__(256) void opt_tail_adamw_kernel(float* __restrict__ p, const G* __restrict__ g, S* __restrict__ m,
                                                             S* __restrict__ v, __bf16* __restrict__ shadow, long n_decay, long n_plain,
                                                             float* __restrict__ hp, double* __restrict__ acc,
                                                             const float* __restrict__ gnorm, float weight_decay) {
    const float gn = gnorm[0];
    const bool finite = gn == gn && fabsf(gn) != INFINITY;
    if (finite) {
        const float lr = hp[VITAE_HP_LR], b1 = hp[VITAE_HP_BETA1], b2 = hp[VITAE_HP_BETA2], eps = hp[VITAE_HP_EPS];
        float bc1 = hp[VITAE_HP_BC1], bc2 = hp[VITAE_HP_BC2];
        const float omb1 = one_minus_beta(bc1, b1), omb2 = one_minus_beta(bc2, b2);
        if (bc1 <= 0.f) {
            const float t = hp[VITAE_HP_STEP] + 1.f;
            device_bias_corrections(omb1, omb2, t, bc1, bc2);
        }
        const float sq_bc2 = sqrtf(bc2), gs = hp[VITAE_HP_GRAD_MUL], step = lr / bc1;
        const long n = n_decay + n_plain;                  // both segment lengths are multiples of 4 (arena alignment)
        for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (long)gridDim.x * 1024) {
            const float decay = adamw_decay(lr, i < n_decay ? weight_decay : 0.f);
            f32x4 pp = *reinterpret_cast<f32x4*>(p + i), mm = state4_ld<S>(m, i / 4), vv = state4_ld<S>(v, i / 4);
            const f32x4 gg = grad4<G>(g, i / 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pp[e], me = mm[e], ve = vv[e];
                adamw_element(pe, me, ve, gg[e], gs, decay, omb1, b2, omb2, step, sq_bc2, eps);
                pp[e] = pe; mm[e] = me; vv[e] = ve;
            }
            *reinterpret_cast<f32x4*>(p + i) = pp;
            state4_st<S>(m, i / 4, mm);
            state4_st<S>(v, i / 4, vv);
            if (shadow) {
                bf16x4 sh;
#pragma unroll
                for (int e = 0; e < 4; ++e) sh[e] = (__bf16)pp[e];
                *reinterpret_cast<bf16x4*>(shadow + i) = sh;
            }
        }
    }
    // the LAST workgroup to get here counts the step (every workgroup has read hp[STEP] by then)
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool last = atomicAdd(reinterpret_cast<int*>(acc + VITAE_ACC_TICKET_B), 1) == (int)gridDim.x - 1;
        if (last && finite) hp[VITAE_HP_STEP] += 1.f;
    }
}

// ---- the head of a step: hp upload from the pinned ring, masking noise, zeroing — one launch inside the captured step
__device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__global__ __launch_bounds__(256) void step_prologue_kernel(float* __restrict__ hp, const float* __restrict__ ring, int slots,
                                                            const long long* __restrict__ seq, float* __restrict__ noise, long n_noise,
                                                            unsigned long long seed, double* __restrict__ acc,
                                                            unsigned int* __restrict__ zp, long zwords) {
    const long long s = *seq;
    const float* src = ring + (s % slots) * VITAE_HP_COUNT;      // pinned host memory, read over the link (64 bytes)
    if (blockIdx.x == 0) {
        if (threadIdx.x < VITAE_HP_HOST_COUNT) hp[threadIdx.x] = src[threadIdx.x];
        for (int i = threadIdx.x; i < VITAE_ACC_COUNT; i += 256) acc[i] = 0.0;
    }
    const long tid = (long)blockIdx.x * 256 + threadIdx.x, nth = (long)gridDim.x * 256;
    if (noise && src[VITAE_HP_NOISE_KEEP] == 0.f) {
        // four uniforms per Philox call: counter = (group index, step sequence number), key = seed; [0, 1) with 24 random bits
        for (long i = tid; i * 4 < n_noise; i += nth) {
            unsigned r[4];
            philox4x32_10((unsigned)seed, (unsigned)(seed >> 32), (unsigned)i, (unsigned)(i >> 32), (unsigned)s, (unsigned)(s >> 32), r);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i * 4 + e < n_noise) noise[i * 4 + e] = (float)(r[e] >> 8) * (1.0f / 16777216.0f);
        }
    }
    if (zp) {
        const long n4 = zwords / 4;
        u32x4_t* z4 = reinterpret_cast<u32x4_t*>(zp);
        const u32x4_t z = {0u, 0u, 0u, 0u};
        for (long i = tid; i < n4; i += nth) z4[i] = z;
        if (blockIdx.x == 0) for (long i = n4 * 4 + threadIdx.x; i < zwords; i += 256) zp[i] = 0u;
    }
}

__global__ void step_epilogue_kernel(long long* __restrict__ seq) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *seq += 1;
}

// ---- multi-tensor AdamW (ABI 54): fine-tuning's separate parameters in layer-decay groups, two launches per step
struct MultiEntry { float* p; const float* g; float* m; float* v; long long n; long long group; };
static_assert(sizeof(MultiEntry) == 8 * VITAE_MULTI_ENTRY_WORDS, "table entry layout (vitae_hip.h)");

// Squares are formed and summed in double (a product of two floats is exact there): what is left of the norm's error is the final
// rounding to fp32.  Read-only, so four workgroups per CU keep enough bytes in flight without unrolling.
__global__ __launch_bounds__(256) void grad_sqnorm_multi_kernel(const MultiEntry* __restrict__ table, const int* __restrict__ chunks,
                                                                long n_chunks, long chunk, double* __restrict__ acc) {
    __shared__ double red[4];
    double s = 0.0;
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const MultiEntry e = table[chunks[2 * c]];
        const long off = (long)chunks[2 * c + 1] * chunk;
        const float* g = e.g + off;
        const long len = e.n - off < chunk ? e.n - off : chunk;
        long done = 0;
        if (!((uintptr_t)g & 15)) {
            const long n4 = len / 4;
            for (long i = threadIdx.x; i < n4; i += 256) {
                const f32x4 v = grad4<float>(g, i);
                s += (double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2] + (double)v[3] * v[3];
            }
            done = n4 * 4;
        }
        for (long i = done + threadIdx.x; i < len; i += 256) s += (double)g[i] * g[i];
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(gradsq_slot(acc), red[0] + red[1] + red[2] + red[3]);
}

// adamw_kernel's data path (U independent 16-byte groups per thread, non-temporal moments and gradients) over one chunk at a time.
// SH (ABI 57): shadow[t] is the device address of tensor t's bf16 copy (0: none), written with cast_bf16_kernel's conversion from the
// parameter values just stored — 16-byte path when the shadow is 8-byte aligned too, else element by element.  A compile-time flag:
// without it the body is the kernel of ABI 54, instruction for instruction.
template <int U, bool SH>
__device__ __forceinline__ void adamw_multi_body(const MultiEntry* table, const int* chunks, long n_chunks,
                                                 long chunk, const float* group_lr,
                                                 const float* group_wd, float omb1, float b2, float omb2, float eps,
                                                 float max_norm, float* state, double* acc,
                                                 float* norm_out, const long long* shadow) {
    __shared__ int last;
    // the norm straight from the accumulator, as adamw_kernel's gacc gate: every wave sums the spread slots itself
    double q = acc[VITAE_ACC_SQ_BASE + (threadIdx.x & 63) * VITAE_ACC_SQ_STRIDE];
    if ((threadIdx.x & 63) == 0) q += acc[VITAE_ACC_GRADSQ];
#pragma unroll
    for (int d = 32; d; d >>= 1) q += __shfl_xor(q, d, 64);
    const float gn = (float)sqrt(q);
    const bool finite = gn == gn && fabsf(gn) != INFINITY;
    const float t = state[VITAE_MULTI_STATE_STEP] + 1.f;
    if (finite) {
        float bc1, bc2;
        device_bias_corrections(omb1, omb2, t, bc1, bc2);
        const float sq_bc2 = sqrtf(bc2);
        const float gs = max_norm > 0.f ? fminf(1.f, max_norm / (gn + 1e-6f)) : 1.f;      // torch.nn.utils.clip_grad_norm_
        for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
            const int t_idx = chunks[2 * c];
            const MultiEntry e = table[t_idx];
            const long off = (long)chunks[2 * c + 1] * chunk;
            const long len = e.n - off < chunk ? e.n - off : chunk;
            const float lr = group_lr[e.group];
            const float decay = adamw_decay(lr, group_wd[e.group]), step = lr / bc1;
            float* p = e.p + off;
            const float* g = e.g + off;
            float *m = e.m + off, *v = e.v + off;
            __bf16* sh = nullptr;
            if constexpr (SH) {
                const long long a = shadow[t_idx];
                if (a) sh = reinterpret_cast<__bf16*>(a) + off;
            }
            long done = 0;
            // chunk and off are multiples of 4: the chunk is 16-byte aligned exactly when the tensor's base addresses are (and its
            // shadow 8-byte aligned exactly when the shadow's base address is)
            if (!(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) && !((uintptr_t)sh & 7)) {
                const long n4 = len / 4;
                f32x4* p4 = reinterpret_cast<f32x4*>(p);
                for (long i0 = threadIdx.x; i0 < n4; i0 += U * 256) {
                    long idx[U];
                    bool live[U];
                    f32x4 pp[U], mm[U], vv[U], gg[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        live[u] = i0 + u * 256 < n4;
                        idx[u] = live[u] ? i0 + u * 256 : i0;
                        pp[u] = p4[idx[u]];
                        mm[u] = state4_ld<float>(m, idx[u]);
                        vv[u] = state4_ld<float>(v, idx[u]);
                        gg[u] = grad4<float>(g, idx[u]);
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (!live[u]) break;
                        const long i = idx[u];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            float pe = pp[u][k], me = mm[u][k], ve = vv[u][k];
                            adamw_element(pe, me, ve, gg[u][k], gs, decay, omb1, b2, omb2, step, sq_bc2, eps);
                            pp[u][k] = pe; mm[u][k] = me; vv[u][k] = ve;
                        }
                        p4[i] = pp[u];
                        state4_st<float>(m, i, mm[u]);
                        state4_st<float>(v, i, vv[u]);
                        if (SH && sh) {
                            bf16x4 h;
#pragma unroll
                            for (int k = 0; k < 4; ++k) h[k] = (__bf16)pp[u][k];
                            reinterpret_cast<bf16x4*>(sh)[i] = h;
                        }
                    }
                }
                done = n4 * 4;
            }
            for (long i = done + threadIdx.x; i < len; i += 256) {
                float pe = p[i], me = m[i], ve = v[i];
                adamw_element(pe, me, ve, g[i], gs, decay, omb1, b2, omb2, step, sq_bc2, eps);
                p[i] = pe; m[i] = me; v[i] = ve;
                if (SH && sh) sh[i] = (__bf16)pe;
            }
        }
    }
    // the LAST workgroup to get here (every one has read the accumulator and state[STEP] by then) publishes the norm, counts the step
    // and leaves the accumulator as it found it before the norm pass: zero
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(reinterpret_cast<int*>(acc + VITAE_ACC_TICKET_B), 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (last && threadIdx.x < 64) {
        acc[VITAE_ACC_SQ_BASE + threadIdx.x * VITAE_ACC_SQ_STRIDE] = 0.0;
        if (threadIdx.x == 0) {
            acc[VITAE_ACC_GRADSQ] = 0.0;
            acc[VITAE_ACC_TICKET_B] = 0.0;
            norm_out[0] = gn;
            state[finite ? VITAE_MULTI_STATE_STEP : VITAE_MULTI_STATE_SKIPPED] += 1.f;
        }
    }
}

template <int U>
__global__ __launch_bounds__(256) void adamw_multi_kernel(const MultiEntry* __restrict__ table, const int* __restrict__ chunks, long n_chunks,
                                                          long chunk, const float* __restrict__ group_lr,
                                                          const float* __restrict__ group_wd, float omb1, float b2, float omb2, float eps,
                                                          float max_norm, float* __restrict__ state, double* __restrict__ acc,
                                                          float* __restrict__ norm_out) {
    adamw_multi_body<U, false>(table, chunks, n_chunks, chunk, group_lr, group_wd, omb1, b2, omb2, eps, max_norm, state, acc, norm_out, nullptr);
}

template <int U>
__global__ __launch_bounds__(256) void adamw_multi_shadow_kernel(const MultiEntry* __restrict__ table, const int* __restrict__ chunks,
                                                                 long n_chunks, long chunk, const float* __restrict__ group_lr,
                                                                 const float* __restrict__ group_wd, float omb1, float b2, float omb2,
                                                                 float eps, float max_norm, float* __restrict__ state,
                                                                 double* __restrict__ acc, float* __restrict__ norm_out,
                                                                 const long long* __restrict__ shadow) {
    adamw_multi_body<U, true>(table, chunks, n_chunks, chunk, group_lr, group_wd, omb1, b2, omb2, eps, max_norm, state, acc, norm_out, shadow);
}

}  // namespace

template <typename G>
static int grad_sqnorm_launch(const G* grads, long n, double* acc, float* norm_out, void* stream) {
    if (!grads || !acc || n <= 0 || ((uintptr_t)grads & 15)) return VITAE_ERR_INVALID_ARG;
    long blocks = (n / 4 + 255) / 256;
    constexpr long maxg = 2048;
    if (blocks > maxg) blocks = maxg;
    if (blocks < 1) blocks = 1;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sqnorm_kernel<G>, dim3((int)blocks), dim3(256), 0, st, grads, n, acc);
    if (norm_out) hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(64), 0, st, acc, norm_out);
    return vitae_launch_status();
}

extern "C" int vitae_grad_norm_finalize(const double* acc, float* norm_out, void* stream) {
    if (!acc || !norm_out) return VITAE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, acc, norm_out);
    return vitae_launch_status();
}

extern "C" int vitae_grad_sqnorm(const float* grads, long n, double* acc, float* norm_out, void* stream) {
    return grad_sqnorm_launch<float>(grads, n, acc, norm_out, stream);
}

extern "C" int vitae_grad_sqnorm_bf16(const void* grads_bf16, long n, double* acc, float* norm_out, void* stream) {
    return grad_sqnorm_launch<__bf16>(reinterpret_cast<const __bf16*>(grads_bf16), n, acc, norm_out, stream);
}

template <typename G, typename S = float>
static int adamw_launch(float* params, const G* grads, S* exp_avg, S* exp_avg_sq, void* shadow_bf16, long n,
                        const float* hp, const float* grad_norm, float weight_decay, void* stream, const double* gacc = nullptr) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !hp || n <= 0) return VITAE_ERR_INVALID_ARG;
    if (((uintptr_t)params & 15) || (((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & (4 * sizeof(S) - 1))) return VITAE_ERR_INVALID_ARG;
    if (((uintptr_t)grads & (4 * sizeof(G) - 1)) || ((uintptr_t)shadow_bf16 & 7)) return VITAE_ERR_INVALID_ARG;
    long blocks = (n / 4 + 255) / 256;
    // one 256-thread workgroup per CU: as fast alone as any larger grid (5.4-5.7 TB/s) and it leaves the CUs' other wave
    // slots to the backward kernels this pass runs beside (in-backward optimiser); fewer workgroups lose bandwidth
    constexpr long maxb = 256;
    if (blocks > maxb) blocks = maxb;
    if (blocks < 1) blocks = 1;
    // 30 B/element of HBM traffic; 5.0-5.7 TB/s for every grid size >= 256 workgroups and cache policy tried (the
    // read-only grad-norm pass reaches 5.4 TB/s on the same box), i.e. this kernel sits at the achievable HBM rate.
    // groups in flight per thread: 2 -> 8 took the pass from 5.0 to 6.1 TB/s alone and the step from 5.58 to 5.18 ms (it
    // spends less time beside the backward kernels it slows down); 12 and 16 are slower again (5.21 / 5.32 ms)
    constexpr int unroll = 8;
    hipLaunchKernelGGL((adamw_kernel<true, G, unroll, S>), dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, reinterpret_cast<__bf16*>(shadow_bf16), n, hp, grad_norm, weight_decay, gacc);
    return vitae_launch_status();
}

// bf16 moments (round 6): the same pass at 22 instead of 30 bytes per parameter.  grads: fp32, or the bf16 wire copy when grads_bf16.
extern "C" int vitae_adamw_step_s16(float* params, const void* grads, int grads_bf16, void* exp_avg_bf16, void* exp_avg_sq_bf16,
                                    void* shadow_bf16, long n, const float* hp, const float* grad_norm, float weight_decay, void* stream) {
    __bf16* m = reinterpret_cast<__bf16*>(exp_avg_bf16);
    __bf16* v = reinterpret_cast<__bf16*>(exp_avg_sq_bf16);
    if (grads_bf16)
        return adamw_launch<__bf16, __bf16>(params, reinterpret_cast<const __bf16*>(grads), m, v, shadow_bf16, n, hp, grad_norm, weight_decay, stream);
    return adamw_launch<float, __bf16>(params, reinterpret_cast<const float*>(grads), m, v, shadow_bf16, n, hp, grad_norm, weight_decay, stream);
}

// ... gated by the gradient-norm accumulator itself (acc: the double[VITAE_ACC_COUNT] block; the step is skipped when the sum of
// acc[VITAE_ACC_GRADSQ] and the VITAE_ACC_SQ_* slots is not finite — what vitae_grad_norm_finalize + grad_norm would say, without that launch)
extern "C" int vitae_adamw_step_s16_acc(float* params, const void* grads, int grads_bf16, void* exp_avg_bf16, void* exp_avg_sq_bf16,
                                        void* shadow_bf16, long n, const float* hp, const double* acc, float weight_decay, void* stream) {
    if (!acc) return VITAE_ERR_INVALID_ARG;
    __bf16* m = reinterpret_cast<__bf16*>(exp_avg_bf16);
    __bf16* v = reinterpret_cast<__bf16*>(exp_avg_sq_bf16);
    if (grads_bf16)
        return adamw_launch<__bf16, __bf16>(params, reinterpret_cast<const __bf16*>(grads), m, v, shadow_bf16, n, hp, nullptr, weight_decay, stream, acc);
    return adamw_launch<float, __bf16>(params, reinterpret_cast<const float*>(grads), m, v, shadow_bf16, n, hp, nullptr, weight_decay, stream, acc);
}

extern "C" int vitae_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                void* shadow_bf16, long n, const float* hp, const float* grad_norm,
                                float weight_decay, void* stream) {
    return adamw_launch<float>(params, grads, exp_avg, exp_avg_sq, shadow_bf16, n, hp, grad_norm, weight_decay, stream);
}

extern "C" int vitae_adamw_step_bf16g(float* params, const void* grads_bf16, float* exp_avg, float* exp_avg_sq,
                                      void* shadow_bf16, long n, const float* hp, const float* grad_norm,
                                      float weight_decay, void* stream) {
    return adamw_launch<__bf16>(params, reinterpret_cast<const __bf16*>(grads_bf16), exp_avg, exp_avg_sq, shadow_bf16, n, hp,
                                grad_norm, weight_decay, stream);
}

extern "C" int vitae_opt_count_bump(float* hp, const float* grad_norm, void* stream) {
    if (!hp) return VITAE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(opt_count_bump_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, hp, grad_norm);
    return vitae_launch_status();
}

extern "C" int vitae_opt_tail(float* params, const void* grads, int grads_bf16, void* exp_avg, void* exp_avg_sq, int state_bf16, void* shadow_bf16,
                              long n_decay, long n_plain, float* hp, double* acc, float* norm_out, float weight_decay, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !hp || !acc || !norm_out || n_decay < 0 || n_plain < 0 || n_decay + n_plain <= 0)
        return VITAE_ERR_INVALID_ARG;
    const uintptr_t smask = state_bf16 ? 7 : 15;
    if ((n_decay & 3) || (n_plain & 3) || (((uintptr_t)params | (uintptr_t)grads) & 15) || (((uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & smask) ||
        ((uintptr_t)shadow_bf16 & 7))
        return VITAE_ERR_UNSUPPORTED_SHAPE;
    const long n = n_decay + n_plain;
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 256) blocks = 256;
    hipStream_t st = (hipStream_t)stream;
    __bf16* sh = reinterpret_cast<__bf16*>(shadow_bf16);
    float *m32 = reinterpret_cast<float*>(exp_avg), *v32 = reinterpret_cast<float*>(exp_avg_sq);
    __bf16 *m16 = reinterpret_cast<__bf16*>(exp_avg), *v16 = reinterpret_cast<__bf16*>(exp_avg_sq);
    if (grads_bf16) {
        const __bf16* g = reinterpret_cast<const __bf16*>(grads);
        hipLaunchKernelGGL(opt_tail_norm_kernel<__bf16>, dim3((int)blocks), dim3(256), 0, st, g, n, acc, norm_out);
        if (state_bf16) hipLaunchKernelGGL((opt_tail_adamw_kernel<__bf16, __bf16>), dim3((int)blocks), dim3(256), 0, st, params, g, m16, v16, sh, n_decay, n_plain, hp, acc, norm_out, weight_decay);
        else hipLaunchKernelGGL((opt_tail_adamw_kernel<__bf16, float>), dim3((int)blocks), dim3(256), 0, st, params, g, m32, v32, sh, n_decay, n_plain, hp, acc, norm_out, weight_decay);
    } else {
        const float* g = reinterpret_cast<const float*>(grads);
        hipLaunchKernelGGL(opt_tail_norm_kernel<float>, dim3((int)blocks), dim3(256), 0, st, g, n, acc, norm_out);
        if (state_bf16) hipLaunchKernelGGL((opt_tail_adamw_kernel<float, __bf16>), dim3((int)blocks), dim3(256), 0, st, params, g, m16, v16, sh, n_decay, n_plain, hp, acc, norm_out, weight_decay);
        else hipLaunchKernelGGL((opt_tail_adamw_kernel<float, float>), dim3((int)blocks), dim3(256), 0, st, params, g, m32, v32, sh, n_decay, n_plain, hp, acc, norm_out, weight_decay);
    }
    return vitae_launch_status();
}

extern "C" int vitae_step_prologue(float* hp, const float* hp_ring, int ring_slots, const long long* step_seq, float* noise, long n_noise,
                                   long long seed, double* acc, void* zero_ptr, long zero_bytes, void* stream) {
    if (!hp || !hp_ring || ring_slots <= 0 || !step_seq || !acc || n_noise < 0 || zero_bytes < 0 || (zero_bytes & 3) ||
        ((uintptr_t)zero_ptr & 15))
        return VITAE_ERR_INVALID_ARG;
    const long work = (n_noise / 4 > zero_bytes / 16 ? n_noise / 4 : zero_bytes / 16);
    long blocks = (work + 255) / 256;
    if (blocks > 512) blocks = 512;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(step_prologue_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, hp, hp_ring, ring_slots, step_seq,
                       noise, n_noise, (unsigned long long)seed, acc, reinterpret_cast<unsigned int*>(zero_ptr), zero_bytes / 4);
    return vitae_launch_status();
}

extern "C" int vitae_step_epilogue(long long* step_seq, void* stream) {
    if (!step_seq) return VITAE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(step_epilogue_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step_seq);
    return vitae_launch_status();
}

// ---- multi-tensor AdamW: the whole call is judged on the host copies before the first launch
static int multi_check(const long long* table, long n_entries, const int* chunks, long n_chunks, long chunk, int n_groups, bool all_ptrs) {
    if (n_entries < 0 || n_chunks < 0 || chunk <= 0 || (chunk & 3)) return VITAE_ERR_INVALID_ARG;
    if (n_entries == 0 || n_chunks == 0) return VITAE_OK;
    if (!table || !chunks) return VITAE_ERR_INVALID_ARG;
    for (long t = 0; t < n_entries; ++t) {
        const long long* e = table + t * VITAE_MULTI_ENTRY_WORDS;
        if (!e[1] || e[4] < 0) return VITAE_ERR_INVALID_ARG;
        if (all_ptrs && (!e[0] || !e[2] || !e[3] || e[5] < 0 || e[5] >= n_groups)) return VITAE_ERR_INVALID_ARG;
    }
    for (long c = 0; c < n_chunks; ++c) {
        const long t = chunks[2 * c], k = chunks[2 * c + 1];
        if (t < 0 || t >= n_entries || k < 0 || (long long)k * chunk >= table[t * VITAE_MULTI_ENTRY_WORDS + 4]) return VITAE_ERR_INVALID_ARG;
    }
    return VITAE_OK;
}

extern "C" int vitae_grad_sqnorm_multi(const long long* table_host, const long long* table_dev, long n_entries, const int* chunks_host,
                                       const int* chunks_dev, long n_chunks, long chunk, double* acc, void* stream) {
    const int rc = multi_check(table_host, n_entries, chunks_host, n_chunks, chunk, 0, false);
    if (rc != VITAE_OK || n_entries == 0 || n_chunks == 0) return rc;
    if (!table_dev || !chunks_dev || !acc) return VITAE_ERR_INVALID_ARG;
    const long blocks = n_chunks < 1024 ? n_chunks : 1024;
    hipLaunchKernelGGL(grad_sqnorm_multi_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const MultiEntry*>(table_dev), chunks_dev, n_chunks, chunk, acc);
    return vitae_launch_status();
}

extern "C" int vitae_adamw_multi(const long long* table_host, const long long* table_dev, long n_entries, const int* chunks_host,
                                 const int* chunks_dev, long n_chunks, long chunk, const float* group_lr_dev, const float* group_wd_dev, int n_groups,
                                 double beta1, double beta2, double eps, double max_norm, float* state, double* acc, float* norm_out,
                                 void* stream) {
    if (n_groups < 1 || n_groups > VITAE_MULTI_MAX_GROUPS || !group_lr_dev || !group_wd_dev) return VITAE_ERR_INVALID_ARG;
    const int rc = multi_check(table_host, n_entries, chunks_host, n_chunks, chunk, n_groups, true);
    if (rc != VITAE_OK || n_entries == 0 || n_chunks == 0) return rc;
    if (!table_dev || !chunks_dev || !state || !acc || !norm_out) return VITAE_ERR_INVALID_ARG;
    // one 256-thread workgroup per CU, as adamw_launch (and for its reasons); the chunk list deals the tensors out evenly
    const long blocks = n_chunks < 256 ? n_chunks : 256;
    // 1 - beta from the host's doubles: what a negative VITAE_HP_BC slot carries for adamw_kernel
    hipLaunchKernelGGL(adamw_multi_kernel<8>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const MultiEntry*>(table_dev), chunks_dev, n_chunks, chunk, group_lr_dev, group_wd_dev, (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)eps, (float)max_norm, state, acc, norm_out);
    return vitae_launch_status();
}

// ... and the bf16 copy of every updated tensor that lists one (ABI 57): 30 instead of 28 bytes per parameter, no cast launch afterwards
extern "C" int vitae_adamw_multi_shadow(const long long* table_host, const long long* table_dev, long n_entries, const int* chunks_host,
                                        const int* chunks_dev, long n_chunks, long chunk, const float* group_lr_dev, const float* group_wd_dev,
                                        int n_groups, double beta1, double beta2, double eps, double max_norm, float* state, double* acc,
                                        float* norm_out, const long long* shadow_host, const long long* shadow_dev, void* stream) {
    if (!shadow_host && !shadow_dev)
        return vitae_adamw_multi(table_host, table_dev, n_entries, chunks_host, chunks_dev, n_chunks, chunk, group_lr_dev, group_wd_dev, n_groups,
                                 beta1, beta2, eps, max_norm, state, acc, norm_out, stream);
    if (!shadow_host || !shadow_dev) return VITAE_ERR_INVALID_ARG;
    if (n_groups < 1 || n_groups > VITAE_MULTI_MAX_GROUPS || !group_lr_dev || !group_wd_dev) return VITAE_ERR_INVALID_ARG;
    const int rc = multi_check(table_host, n_entries, chunks_host, n_chunks, chunk, n_groups, true);
    if (rc != VITAE_OK || n_entries == 0 || n_chunks == 0) return rc;
    if (!table_dev || !chunks_dev || !state || !acc || !norm_out) return VITAE_ERR_INVALID_ARG;
    for (long t = 0; t < n_entries; ++t)
        if (shadow_host[t] & 1) return VITAE_ERR_INVALID_ARG;          // not a bf16 address
    const long blocks = n_chunks < 256 ? n_chunks : 256;               // vitae_adamw_multi's grid
    hipLaunchKernelGGL(adamw_multi_shadow_kernel<8>, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const MultiEntry*>(table_dev), chunks_dev, n_chunks, chunk, group_lr_dev, group_wd_dev, (float)(1.0 - beta1),
                       (float)beta2, (float)(1.0 - beta2), (float)eps, (float)max_norm, state, acc, norm_out, shadow_dev);
    return vitae_launch_status();
}

namespace {
// Own fill kernel instead of hipMemsetAsync: as a captured graph memset node the latter left a few words
// of a 787 KB region unwritten on ROCm 7.2 (seen as garbage in the cls_token gradient under graph replay).
__global__ __launch_bounds__(256) void zero_kernel(unsigned int* __restrict__ p, long nwords) {
    const long n4 = nwords / 4;
    u32x4_t* p4 = reinterpret_cast<u32x4_t*>(p);
    const u32x4_t z = {0u, 0u, 0u, 0u};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) p4[i] = z;
    if (blockIdx.x == 0) for (long i = n4 * 4 + threadIdx.x; i < nwords; i += 256) p[i] = 0u;
}
}  // namespace

extern "C" int vitae_memset_zero(void* ptr, long bytes, void* stream) {
    if (!ptr || bytes < 0 || (bytes & 3) || ((uintptr_t)ptr & 15)) return VITAE_ERR_INVALID_ARG;
    if (bytes == 0) return VITAE_OK;
    const long nwords = bytes / 4;
    long blocks = (nwords / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(zero_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<unsigned int*>(ptr), nwords);
    return vitae_launch_status();
}

extern "C" int vitae_abi_version(void) { return VITAE_ABI_VERSION; }

extern "C" const char* vitae_build_arch(void) { return "gfx950"; }
