// 3-D ResNet baseline (k_fold_training_scripts/resnet_3d.py): Conv3d forward / input gradient / weight gradient as gather-GEMMs on
// v_mfma_f32_32x32x16_bf16, MaxPool3d(3, 2, 1), the global average pool, and the packing of their operands.
//
// Activations are channels-last [N, D, H, W, C] = rows x channels, so a convolution is C[M, Cout] = A[M, K] B[Cout, K]^T with
// K = taps * Cin and A never materialised: every lane gathers the 8 k-values of its MFMA fragment straight from the activation
// (one 16-byte load when Cin % 8 == 0, two 8-byte loads when Cin % 4 == 0, element by element otherwise: the 1-channel stem).
// The input gradient is the SAME kernel with the coordinate rule turned round (source = dy16, a tap contributes when the stride
// divides the offset) and the transposed packed weight.  The weight gradient reduces over the rows M in chunks of
// VITAE_CONV3D_WGRAD_CHUNK: a partial per chunk into the caller's workspace, summed in chunk order by a second launch.
//
// MFMA operand maps (32x32x16 bf16): lane l, r = l & 31, h = l >> 5 holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r], j = 0..7;
// the result has col = l & 31 and row = (reg & 3) + 8 (reg >> 2) + 4 h.
//
// Two routes share every kernel body here through an operand policy (OpBf16, OpX3 below).  bf16: sources and packed weight are bf16,
// one MFMA per k-step.  fp32x3: every fp32 value v enters the bf16 MFMA as two halves, hi = bf16(v) and lo = bf16(v - float(hi)), so
// v is carried to ~2^-16 relative instead of 2^-8.  A product is formed as three terms into ONE accumulator, in this fixed order per
// k-step:
//
//     acc = mfma(a_lo, b_hi, acc);   acc = mfma(a_hi, b_lo, acc);   acc = mfma(a_hi, b_hi, acc);      (cross terms first, then hi.hi)
//
// lo.lo (<= 2^-16 of the product) is dropped.  a = the gathered row operand: the route's fp32 channels-last activation or gradient,
// split in registers by the lane that gathered it — no producer writes extra planes (32 bytes as two 16-byte loads of consecutive
// addresses when Cin % 8 == 0, 16 bytes when Cin % 4 == 0, else element by element).  b = the weight, packed once per optimiser step
// as two bf16 planes per row, [hi (Kp) | lo (Kp)], in the same k = tap * inner + c order with zero tails.  The weight gradient splits
// both of its fp32 operands (dy, x) in registers.  A non-finite fp32 source gives a NaN lo half (inf - inf), so it poisons what reads it.
//
// Safety: a gather is issued only under its predicate (row in range, k < K, source voxel inside the volume), so no address outside
// an operand is formed; offsets are 64-bit.  No LDS beyond a 343-entry tap table / a 64-row coordinate table.
#include "common.hpp"
#include "vitae_hip.h"

#include <limits.h>
#include <initializer_list>

namespace {

constexpr int KSTEP = VITAE_CONV3D_K_STEP;
constexpr int MAX_TAPS = 7 * 7 * 7;
constexpr int WCHUNK = VITAE_CONV3D_WGRAD_CHUNK;
// Two-level accumulation: the MFMA chain runs FLUSH k-steps (128 k-values; three MFMAs each on the fp32x3 route) in fp32 and is then
// added to a double total.  One fp32 chain over the stem's 1372 steps (all products of one sign) was 18 ulp off in the worst element,
// 4.6 x torch's blocked fp32 sum.
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

// ------------------------------------------------------------------ operand policies: all that differs between the two routes
// Src: the element of the gathered operands.  PLANES: bf16 planes of Kp per packed weight row.  AFrag / BFrag: the 8 k-values of a
// lane as gathered (indexable by element) / as the packed weight is loaded; both are zero when value-initialised.  gather<G>: the
// g-th group of G consecutive values at p.  mma(a, b, acc): a gathered; b the weight or, in the weight gradient, gathered as well.
struct OpBf16 {
    using Src = __bf16;
    static constexpr int PLANES = 1;
    using AFrag = bf16x8;
    using BFrag = bf16x8;
    static __device__ __forceinline__ BFrag load_b(const __bf16* wrow, int k0, int) { return *reinterpret_cast<const bf16x8*>(wrow + k0); }
    template <int G>
    static __device__ __forceinline__ void gather(AFrag& a, const Src* p, int g) {
        if (G == 8) a = *reinterpret_cast<const bf16x8*>(p);
        else if (G == 4) {
            const bf16x4 q = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) a[4 * g + e] = q[e];
        } else a[g] = *p;
    }
    static __device__ __forceinline__ f32x16 mma(const AFrag& a, const BFrag& b, f32x16 acc) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
};

struct OpX3 {
    using Src = float;
    static constexpr int PLANES = 2;
    struct AFrag {
        float v[8];
        __device__ __forceinline__ float& operator[](int j) { return v[j]; }
    };
    struct BFrag { bf16x8 hi, lo; };
    static __device__ __forceinline__ BFrag load_b(const __bf16* wrow, int k0, int Kp) {
        return {*reinterpret_cast<const bf16x8*>(wrow + k0), *reinterpret_cast<const bf16x8*>(wrow + Kp + k0)};
    }
    template <int G>
    static __device__ __forceinline__ void gather(AFrag& a, const Src* p, int g) {
        if (G == 8) {
            const f32x4 q0 = *reinterpret_cast<const f32x4*>(p), q1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { a.v[e] = q0[e]; a.v[4 + e] = q1[e]; }
        } else if (G == 4) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) a.v[4 * g + e] = q[e];
        } else a.v[g] = *p;
    }
    static __device__ __forceinline__ BFrag split(const AFrag& a) {
        BFrag s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s.hi[j] = (__bf16)a.v[j];
            s.lo[j] = (__bf16)(a.v[j] - (float)s.hi[j]);
        }
        return s;
    }
    static __device__ __forceinline__ f32x16 mma(const BFrag& a, const BFrag& b, f32x16 acc) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.hi, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.lo, acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.hi, acc, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16 mma(const AFrag& a, const BFrag& b, f32x16 acc) { return mma(split(a), b, acc); }
    static __device__ __forceinline__ f32x16 mma(const AFrag& a, const AFrag& b, f32x16 acc) { return mma(split(a), split(b), acc); }
};

// ------------------------------------------------------------------ packing
// the fp32 value at (row, k) of a packed weight: k = tap * inner + c, zero behind K; w is torch's [Cout, Cin, taps]
__device__ __forceinline__ float packed_value(const float* __restrict__ w, int Cout, int Cin, int taps, bool transposed, int row, int k) {
    const int inner = transposed ? Cout : Cin;
    if (k >= taps * inner) return 0.f;
    const int tap = k / inner, c = k % inner;
    const int co = transposed ? c : row, ci = transposed ? row : c;
    return w[((long)co * Cin + ci) * taps + tap];
}

// [rows][Kp] (PLANES = 1) or [rows][hi (Kp) | lo (Kp)] (PLANES = 2)
template <int PLANES>
__global__ __launch_bounds__(256) void conv3d_pack_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int Cout, int Cin, int taps,
                                                          int Kp, int transposed, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;              // over [row][k] of ONE plane
    if (i >= total) return;
    const int row = (int)(i / Kp), k = (int)(i % Kp);
    const float v = packed_value(w, Cout, Cin, taps, transposed, row, k);
    const __bf16 hi = (__bf16)v;
    if (PLANES == 1) out[i] = hi;
    else {
        out[2L * row * Kp + k] = hi;
        out[2L * row * Kp + Kp + k] = (__bf16)(v - (float)hi);
    }
}

// VITAE_OK and the padded row length of one weight, or the refusal
int pack_geo(const float* w, const void* out, int Cout, int Cin, int kd, int kh, int kw, int transposed, long& Kp) {
    if (!w || !out || Cout <= 0 || Cin <= 0) return VITAE_ERR_INVALID_ARG;
    if (kd < 1 || kh < 1 || kw < 1 || kd > 7 || kh > 7 || kw > 7 || (Cout & 3)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    Kp = kpad((long)kd * kh * kw * (transposed ? Cout : Cin));
    return Kp > (long)INT_MAX - 256 ? VITAE_ERR_UNSUPPORTED_SHAPE : VITAE_OK;
}

template <int PLANES>
int run_pack(const float* w, void* out, int Cout, int Cin, int taps, long Kp, int transposed, void* stream) {
    const long total = (long)(transposed ? Cin : Cout) * Kp;
    hipLaunchKernelGGL(conv3d_pack_kernel<PLANES>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, reinterpret_cast<__bf16*>(out), Cout,
                       Cin, taps, (int)Kp, transposed ? 1 : 0, total);
    return vitae_launch_status();
}

// Every operand of a network in one launch: the destinations laid end to end and cut into chunks of PACK_CHUNK elements; chunks[2 c],
// chunks[2 c + 1] = the entry in which chunk c begins and the offset there in groups of 8.  A thread converts 8 consecutive k of one
// row (a packed size is a multiple of 16, so a group lies in one row of one entry), each through packed_value as conv3d_pack_kernel,
// and stores them as 16 bytes; it walks on to the next entry when its group lies behind the current one.  The last word of an entry
// is its form: bit 0 transposed, VITAE_CONV3D_PACK_FORM_X3 two planes per row [hi | lo] (2 Kp elements: the first Kp groups / 8 of a
// row are bf16(w), the others bf16(w - float(bf16(w)))).
static_assert(VITAE_CONV3D_PACK_CHUNK % (8 * 256) == 0, "a chunk is a whole number of groups per thread");
struct PackEntry { const float* w; __bf16* out; long long Cout, Cin, kd, kh, kw, form; };
constexpr long long FORM_X3 = VITAE_CONV3D_PACK_FORM_X3;
constexpr int PACK_GROUPS = VITAE_CONV3D_PACK_CHUNK / 8;

__host__ __device__ inline long pack_entry_groups(const PackEntry& e, int& taps, int& Kp) {
    taps = (int)(e.kd * e.kh * e.kw);
    const bool tr = e.form & 1;
    const long K = (long)taps * (tr ? e.Cout : e.Cin);
    Kp = (int)((K + KSTEP - 1) / KSTEP * KSTEP);
    return (tr ? e.Cin : e.Cout) * (long)Kp / 8 * (e.form & FORM_X3 ? 2 : 1);
}

__global__ __launch_bounds__(256) void conv3d_pack_multi_kernel(const PackEntry* __restrict__ table, int n_entries, const int* __restrict__ chunks,
                                                                long total_groups) {
    const long first = (long)blockIdx.x * PACK_GROUPS;
    const int n = (int)(total_groups - first < PACK_GROUPS ? total_groups - first : PACK_GROUPS);
    int t = chunks[2 * blockIdx.x];
    long start = -(long)chunks[2 * blockIdx.x + 1];       // the chunk-local group at which entry t begins
    PackEntry e = table[t];
    int taps, Kp;
    long groups = pack_entry_groups(e, taps, Kp);
    // Slot j of the chunk is group (j % 16) * (PACK_GROUPS / 16) + j / 16: 16 neighbouring lanes take groups 256 elements apart — for
    // the wide layers one tap apart, neighbouring source addresses — and lanes l, l + 16, l + 32, l + 48 neighbouring groups (64
    // bytes of one destination line).  A thread's groups still ascend, so it only ever walks forward through the table.
    for (int j = threadIdx.x; j < PACK_GROUPS; j += 256) {
        const int i = (j & 15) * (PACK_GROUPS / 16) + (j >> 4);
        if (i >= n) continue;
        while (i - start >= groups) {
            start += groups;
            if (++t >= n_entries) return;                 // (the launcher checked the list: not reached)
            e = table[t];
            groups = pack_entry_groups(e, taps, Kp);
        }
        const long o = (i - start) * 8;
        const bool tr = e.form & 1, x3 = e.form & FORM_X3;
        const long rowlen = x3 ? 2L * Kp : Kp;
        const int row = (int)(o / rowlen), kk = (int)(o % rowlen);
        const bool lo = kk >= Kp;                         // the second plane of a two-plane row
        const int k0 = lo ? kk - Kp : kk;
        bf16x8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = packed_value(e.w, (int)e.Cout, (int)e.Cin, taps, tr, row, k0 + j);
            h[j] = lo ? (__bf16)(v - (float)(__bf16)v) : (__bf16)v;
        }
        *reinterpret_cast<bf16x8*>(e.out + o) = h;
    }
}

template <class T>
__global__ __launch_bounds__(256) void channels_last_kernel(const float* __restrict__ x, T* __restrict__ out, int C, long S, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;      // output index: (n S + s) C + c
    if (i >= total) return;
    const int c = (int)(i % C);
    const long ns = i / C, n = ns / S, s = ns % S;
    out[i] = (T)x[(n * C + c) * S + s];
}

template <class T>
int run_channels_last(const float* x, T* out, int N, int C, int D, int H, int W, void* stream) {
    if (!x || !out || N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return VITAE_ERR_INVALID_ARG;
    const long S = (long)D * H * W, total = (long)N * S * C;
    if (total > (long)INT_MAX * 128) return VITAE_ERR_UNSUPPORTED_SHAPE;
    hipLaunchKernelGGL(channels_last_kernel<T>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, out, C, S, total);
    return vitae_launch_status();
}

// ------------------------------------------------------------------ forward / input gradient: one gather-GEMM
template <class Op>
struct GatherArgs {
    const typename Op::Src* src; const __bf16* wpk; float* out; __bf16* out16;
    int Ds, Hs, Ws, Cs;         // source volume of one sample, its channels
    int Dr, Hr, Wr;             // row space of one sample
    int M, Nout;                // rows, output columns
    int kd, kh, kw, sd, sh, sw, pd, ph, pw;
    int K, Kp, cs_shift;        // K = taps * Cs; Kp = K padded to the k step (one plane of a packed row); log2(Cs) or -1
    int accum;                  // != 0: the result is added to what `out` holds
};

template <class Op, int G, bool BWD>
__global__ __launch_bounds__(256) void conv3d_gather_kernel(const GatherArgs<Op> a) {
    __shared__ int tab[MAX_TAPS];                                    // tap -> kd_i << 16 | kh_i << 8 | kw_i
    const int taps = a.kd * a.kh * a.kw;
    for (int t = threadIdx.x; t < taps; t += 256) {
        const int r = t / a.kw;
        tab[t] = ((r / a.kh) << 16) | ((r % a.kh) << 8) | (t % a.kw);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
    const int row0 = blockIdx.x * 128 + wave * 32;
    const int m = row0 + l31;                                        // the row of this lane's A fragment
    const bool mok = m < a.M;
    int n = 0, bd = 0, bh = 0, bw = 0;
    if (mok) {
        int r = m;
        const int wr = r % a.Wr; r /= a.Wr;
        const int hr = r % a.Hr; r /= a.Hr;
        const int dr = r % a.Dr; n = r / a.Dr;
        bd = BWD ? dr + a.pd : dr * a.sd - a.pd;
        bh = BWD ? hr + a.ph : hr * a.sh - a.ph;
        bw = BWD ? wr + a.pw : wr * a.sw - a.pw;
    }
    const int co = blockIdx.y * 32 + l31;                            // the column of this lane's B fragment
    const bool cok = co < a.Nout;
    const __bf16* wrow = a.wpk + (long)(cok ? co : 0) * ((long)Op::PLANES * a.Kp) + 8 * hi;
    const long nbase = (long)n * a.Ds;

    f32x16 acc;
    double tot[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; tot[i] = 0.; }
    int chain = 0;
    for (int k0 = 0; k0 < a.Kp; k0 += KSTEP) {
        typename Op::AFrag av{};
        typename Op::BFrag bv{};
        if (cok) bv = Op::load_b(wrow, k0, a.Kp);
#pragma unroll
        for (int g = 0; g < 8 / G; ++g) {
            const int k = k0 + 8 * hi + g * G;
            if (!mok || k >= a.K) continue;                          // the zero tail of K: predicated, not multiplied by zero weights
            const int tap = a.cs_shift >= 0 ? k >> a.cs_shift : k / a.Cs;
            const int ci = k - tap * a.Cs;
            const int t = tab[tap];
            int d, h, w;
            const bool ok = conv_axis<BWD>(bd, t >> 16, a.sd, a.Ds, d) & conv_axis<BWD>(bh, (t >> 8) & 255, a.sh, a.Hs, h) &
                            conv_axis<BWD>(bw, t & 255, a.sw, a.Ws, w);
            if (!ok) continue;
            Op::template gather<G>(av, a.src + (((nbase + d) * a.Hs + h) * a.Ws + w) * a.Cs + ci, g);
        }
        acc = Op::mma(av, bv, acc);
        if (++chain == FLUSH) { flush_acc(acc, tot); chain = 0; }
    }
    flush_acc(acc, tot);
    if (!cok) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mm = row0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (mm >= a.M) continue;
        const long o = (long)mm * a.Nout + co;
        float v = (float)tot[r];
        if (a.accum) v += a.out[o];
        if (a.out) a.out[o] = v;
        if (a.out16) a.out16[o] = (__bf16)v;
    }
}

// forward (src = x, out = y) or input gradient (src = dy, wpk = the transposed form, out = dx) of a checked geometry; the launch status
template <class Op, bool BWD>
int run_gather(const ConvGeo& g, const void* src, const void* wpk, float* out, void* out16, int accumulate, void* stream) {
    GatherArgs<Op> a;
    a.src = reinterpret_cast<const typename Op::Src*>(src); a.wpk = reinterpret_cast<const __bf16*>(wpk);
    a.out = out; a.out16 = reinterpret_cast<__bf16*>(out16);
    if (!BWD) { a.Ds = g.D; a.Hs = g.H; a.Ws = g.W; a.Cs = g.Cin; a.Dr = g.Do; a.Hr = g.Ho; a.Wr = g.Wo; a.M = (int)g.M; a.Nout = g.Cout; }
    else { a.Ds = g.Do; a.Hs = g.Ho; a.Ws = g.Wo; a.Cs = g.Cout; a.Dr = g.D; a.Hr = g.H; a.Wr = g.W; a.M = (int)g.V; a.Nout = g.Cin; }
    a.kd = g.kd; a.kh = g.kh; a.kw = g.kw; a.sd = g.sd; a.sh = g.sh; a.sw = g.sw; a.pd = g.pd; a.ph = g.ph; a.pw = g.pw;
    a.K = g.taps * a.Cs; a.Kp = (int)kpad(a.K); a.cs_shift = shift_of(a.Cs); a.accum = accumulate ? 1 : 0;
    const dim3 grid(cdiv(a.M, 128), cdiv(a.Nout, 32));
    const hipStream_t st = (hipStream_t)stream;
    if (a.Cs % 8 == 0) hipLaunchKernelGGL((conv3d_gather_kernel<Op, 8, BWD>), grid, dim3(256), 0, st, a);
    else if (a.Cs % 4 == 0) hipLaunchKernelGGL((conv3d_gather_kernel<Op, 4, BWD>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv3d_gather_kernel<Op, 1, BWD>), grid, dim3(256), 0, st, a);
    return vitae_launch_status();
}

// ------------------------------------------------------------------ weight gradient
// Workgroup = (128 k-columns: 32 per wave) x (32 output channels) x (one chunk of rows).  MFMA: A[row = co][k = m] = dy16[m, co],
// B[k = m][col = kcol] = x16[src(m, tap(kcol)), ci(kcol)].  The 8 rows of a lane's fragments are the same for the 32 lanes of a
// half wave; their decoded coordinates come from a 64-row table in LDS that the first wave refills every 64 rows.  Both operands are
// gathered, element by element (Op::Src; on the fp32x3 route both are split in registers, by Op::mma after the element loop: a split
// inside the loop costs one route or the other registers or instructions, whichever way it is written — LABNOTES.md).
template <class Op>
__global__ __launch_bounds__(256) void conv3d_wgrad_part_kernel(const typename Op::Src* __restrict__ dy16, const typename Op::Src* __restrict__ x16,
                                                                float* __restrict__ ws, const ConvGeo g) {
    __shared__ int4 rowtab[64];                                       // n (or -1 past the chunk), od sd - pd, oh sh - ph, ow sw - pw
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, hi = lane >> 5;
    const int K = (int)g.K, M = (int)g.M;
    const int kcol = blockIdx.x * 128 + wave * 32 + l31;
    const bool kok = kcol < K;
    const int tap = kok ? kcol / g.Cin : 0, ci = kok ? kcol % g.Cin : 0;
    const int tkw = tap % g.kw, tkh = (tap / g.kw) % g.kh, tkd = tap / (g.kw * g.kh);
    const int co = blockIdx.y * 32 + l31;
    const bool cok = co < g.Cout;
    const int m_begin = blockIdx.z * WCHUNK, m_end = min(M, m_begin + WCHUNK);

    f32x16 acc;
    double tot[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; tot[i] = 0.; }
    for (int mb = m_begin; mb < m_end; mb += 64) {
        if (((mb - m_begin) & (FLUSH * KSTEP - 1)) == 0) flush_acc(acc, tot);
        __syncthreads();
        if (threadIdx.x < 64) {
            const int m = mb + threadIdx.x;
            int4 e = make_int4(-1, 0, 0, 0);
            if (m < m_end) {
                int r = m;
                const int ow = r % g.Wo; r /= g.Wo;
                const int oh = r % g.Ho; r /= g.Ho;
                const int od = r % g.Do;
                e = make_int4(r / g.Do, od * g.sd - g.pd, oh * g.sh - g.ph, ow * g.sw - g.pw);
            }
            rowtab[threadIdx.x] = e;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (mb + ks * KSTEP >= m_end) break;                      // uniform over the workgroup
            typename Op::AFrag av, bv;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ml = ks * KSTEP + 8 * hi + j;
                const int4 e = rowtab[ml];
                const bool rok = e.x >= 0;
                const int d = e.y + tkd, h = e.z + tkh, w = e.w + tkw;
                av[j] = 0.f; bv[j] = 0.f;
                if (rok && cok) av[j] = dy16[(long)(mb + ml) * g.Cout + co];
                if (rok && kok && d >= 0 && d < g.D && h >= 0 && h < g.H && w >= 0 && w < g.W)
                    bv[j] = x16[((((long)e.x * g.D + d) * g.H + h) * g.W + w) * g.Cin + ci];
            }
            acc = Op::mma(av, bv, acc);
        }
    }
    flush_acc(acc, tot);
    if (!kok) return;
    const int crow0 = blockIdx.y * 32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = crow0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (c < g.Cout) ws[((long)blockIdx.z * g.Cout + c) * K + kcol] = (float)tot[r];
    }
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

// VITAE_OK and the chunk count of a checked geometry, or the refusal of the caller's workspace
int wgrad_chunks(const ConvGeo& g, long ws_floats, int& chunks) {
    chunks = cdiv(g.M, WCHUNK);
    if (ws_floats < (long)chunks * g.Cout * g.K) return VITAE_ERR_INVALID_ARG;
    if (chunks > 65535) return VITAE_ERR_UNSUPPORTED_SHAPE;                     // grid.z
    return VITAE_OK;
}

template <class Op>
int run_wgrad(const ConvGeo& g, int chunks, const void* dy, const void* x, float* dw, float* ws, int accumulate, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv3d_wgrad_part_kernel<Op>, dim3(cdiv(g.K, 128), cdiv(g.Cout, 32), chunks), dim3(256), 0, st,
                       reinterpret_cast<const typename Op::Src*>(dy), reinterpret_cast<const typename Op::Src*>(x), ws, g);
    const long total = (long)g.Cout * g.K;
    hipLaunchKernelGGL(conv3d_wgrad_sum_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, ws, dw, chunks, g.Cout, g.Cin, g.taps, accumulate ? 1 : 0);
    return vitae_launch_status();
}

// ------------------------------------------------------------------ MaxPool3d(3, 2, 1)
__global__ __launch_bounds__(256) void maxpool3d_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, __bf16* __restrict__ y16,
                                                            unsigned char* __restrict__ idx, int D, int H, int W, int C, int Do, int Ho, int Wo,
                                                            long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;              // (((n Do + od) Ho + oh) Wo + ow) C + c
    if (i >= total) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int ow = (int)(r % Wo); r /= Wo;
    const int oh = (int)(r % Ho); r /= Ho;
    const int od = (int)(r % Do);
    const long n = r / Do;
    float best = -INFINITY;
    int bi = -1;
    for (int a = 0; a < 3; ++a) {
        const int d = od * 2 - 1 + a;
        if (d < 0 || d >= D) continue;
        for (int b = 0; b < 3; ++b) {
            const int h = oh * 2 - 1 + b;
            if (h < 0 || h >= H) continue;
            for (int e = 0; e < 3; ++e) {
                const int w = ow * 2 - 1 + e;
                if (w < 0 || w >= W) continue;
                const float v = x[(((n * D + d) * H + h) * W + w) * C + c];
                // torch's scan: the first position is the start index; a value takes over when it is greater or NaN
                if (bi < 0 || v > best || v != v) { best = v; bi = (a * 3 + b) * 3 + e; }
            }
        }
    }
    if (y) y[i] = best;
    if (y16) y16[i] = (__bf16)best;
    idx[i] = (unsigned char)bi;
}

__global__ __launch_bounds__(256) void maxpool3d_bwd_kernel(const float* __restrict__ dy, const unsigned char* __restrict__ idx, float* __restrict__ dx,
                                                            __bf16* __restrict__ dx16, int D, int H, int W, int C, int Do, int Ho, int Wo, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;              // (((n D + d) H + h) W + w) C + c
    if (i >= total) return;
    const int c = (int)(i % C);
    long r = i / C;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H); r /= H;
    const int d = (int)(r % D);
    const long n = r / D;
    float s = 0.f;
    for (int a = 0; a < 3; ++a) {
        const int td = d + 1 - a;
        if (td < 0 || (td & 1) || (td >> 1) >= Do) continue;
        for (int b = 0; b < 3; ++b) {
            const int th = h + 1 - b;
            if (th < 0 || (th & 1) || (th >> 1) >= Ho) continue;
            for (int e = 0; e < 3; ++e) {
                const int tw = w + 1 - e;
                if (tw < 0 || (tw & 1) || (tw >> 1) >= Wo) continue;
                const long o = (((n * Do + (td >> 1)) * Ho + (th >> 1)) * Wo + (tw >> 1)) * C + c;
                if (idx[o] == (a * 3 + b) * 3 + e) s += dy[o];
            }
        }
    }
    if (dx) dx[i] = s;
    if (dx16) dx16[i] = (__bf16)s;
}

// ------------------------------------------------------------------ global average pool
__global__ __launch_bounds__(256) void rows_mean_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, __bf16* __restrict__ y16, int S, int C,
                                                            long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;              // n C + c
    if (i >= total) return;
    const long n = i / C;
    const int c = (int)(i % C);
    float s = 0.f;
    for (int r = 0; r < S; ++r) s += x[(n * S + r) * C + c];
    const float v = s / (float)S;
    if (y) y[i] = v;
    if (y16) y16[i] = (__bf16)v;
}

__global__ __launch_bounds__(256) void rows_mean_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, __bf16* __restrict__ dx16, int S, int C,
                                                            long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;              // (n S + s) C + c
    if (i >= total) return;
    const long n = i / ((long)S * C);
    const float v = dy[n * C + (int)(i % C)] / (float)S;
    if (dx) dx[i] = v;
    if (dx16) dx16[i] = (__bf16)v;
}

int pool_geo(int N, int D, int H, int W, int C, int& Do, int& Ho, int& Wo, long& in_total, long& out_total) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return VITAE_ERR_INVALID_ARG;
    Do = (D - 1) / 2 + 1; Ho = (H - 1) / 2 + 1; Wo = (W - 1) / 2 + 1;            // (X + 2 - 3) / 2 + 1
    in_total = (long)N * D * H * W * C; out_total = (long)N * Do * Ho * Wo * C;
    if ((long)N * D * H * W > (long)INT_MAX - 256) return VITAE_ERR_UNSUPPORTED_SHAPE;
    return VITAE_OK;
}

}  // namespace

extern "C" long vitae_conv3d_packed_elems(int Cout, int Cin, int kd, int kh, int kw, int transposed) {
    if (Cout <= 0 || Cin <= 0 || kd < 1 || kh < 1 || kw < 1 || kd > 7 || kh > 7 || kw > 7) return 0;
    const long taps = (long)kd * kh * kw;
    return transposed ? Cin * kpad(taps * Cout) : Cout * kpad(taps * Cin);
}

extern "C" int vitae_conv3d_pack_weight(const float* w, void* w16, int Cout, int Cin, int kd, int kh, int kw, int transposed, void* stream) {
    long Kp;
    if (const int rc = pack_geo(w, w16, Cout, Cin, kd, kh, kw, transposed, Kp)) return rc;
    return run_pack<1>(w, w16, Cout, Cin, kd * kh * kw, Kp, transposed, stream);
}

extern "C" long vitae_conv3d_packed_elems_x3(int Cout, int Cin, int kd, int kh, int kw, int transposed) {
    return 2 * vitae_conv3d_packed_elems(Cout, Cin, kd, kh, kw, transposed);
}

extern "C" int vitae_conv3d_pack_weight_x3(const float* w, void* w16x2, int Cout, int Cin, int kd, int kh, int kw, int transposed, void* stream) {
    long Kp;
    if (const int rc = pack_geo(w, w16x2, Cout, Cin, kd, kh, kw, transposed, Kp)) return rc;
    if ((uintptr_t)w16x2 & 15) return VITAE_ERR_UNSUPPORTED_SHAPE;
    return run_pack<2>(w, w16x2, Cout, Cin, kd * kh * kw, Kp, transposed, stream);
}

namespace {
inline long pack_form_elems(int Cout, int Cin, int kd, int kh, int kw, long long form) {
    return vitae_conv3d_packed_elems(Cout, Cin, kd, kh, kw, (int)(form & 1)) * (form & FORM_X3 ? 2 : 1);
}

// VITAE_OK or the refusal of a pack table (host copy); total_groups: all destinations in groups of 8 elements
int pack_multi_check(const long long* table, long n_entries, long& total_groups) {
    if (!table || n_entries <= 0 || n_entries > INT_MAX) return VITAE_ERR_INVALID_ARG;
    total_groups = 0;
    for (long t = 0; t < n_entries; ++t) {
        const long long* w = table + t * VITAE_CONV3D_PACK_ENTRY_WORDS;
        const long long Cout = w[2], Cin = w[3], kd = w[4], kh = w[5], kw = w[6], form = w[7], tr = form & 1;
        if (!w[0] || !w[1] || Cout <= 0 || Cin <= 0 || Cout > INT_MAX || Cin > INT_MAX || (form & ~(1 | FORM_X3))) return VITAE_ERR_INVALID_ARG;
        if (kd < 1 || kh < 1 || kw < 1 || kd > 7 || kh > 7 || kw > 7 || (Cout & 3)) return VITAE_ERR_UNSUPPORTED_SHAPE;
        if (w[1] & 15) return VITAE_ERR_UNSUPPORTED_SHAPE;
        if (kpad(kd * kh * kw * (tr ? Cout : Cin)) > (long)INT_MAX - 256) return VITAE_ERR_UNSUPPORTED_SHAPE;
        const long elems = pack_form_elems((int)Cout, (int)Cin, (int)kd, (int)kh, (int)kw, form);
        if (elems <= 0 || elems > VITAE_CONV3D_PACK_MAX_ELEMS) return VITAE_ERR_UNSUPPORTED_SHAPE;
        total_groups += elems / 8;
        if (total_groups * 8 > VITAE_CONV3D_PACK_MAX_ELEMS) return VITAE_ERR_UNSUPPORTED_SHAPE;
    }
    return VITAE_OK;
}

// the chunk list of a checked table: written to `out` (check == NULL) or compared with `check`
bool pack_multi_walk(const long long* table, long n_entries, long n_chunks, int* out, const int* check) {
    const auto groups_of = [&](long t) {
        const long long* w = table + t * VITAE_CONV3D_PACK_ENTRY_WORDS;
        return pack_form_elems((int)w[2], (int)w[3], (int)w[4], (int)w[5], (int)w[6], w[7]) / 8;
    };
    long t = 0, off = 0, groups = groups_of(0);           // where the next chunk begins: entry, group offset inside it
    for (long c = 0; c < n_chunks; ++c) {
        if (t >= n_entries) return false;
        if (check) { if (check[2 * c] != (int)t || check[2 * c + 1] != (int)off) return false; }
        else { out[2 * c] = (int)t; out[2 * c + 1] = (int)off; }
        long left = PACK_GROUPS;
        while (left > 0 && t < n_entries) {
            const long take = groups - off < left ? groups - off : left;
            off += take; left -= take;
            if (off == groups) {
                off = 0;
                if (++t < n_entries) groups = groups_of(t);
            }
        }
    }
    return t == n_entries;                                // the list covers every entry, no more
}
}  // namespace

extern "C" long vitae_conv3d_pack_multi_chunks(const long long* table_host, long n_entries) {
    long total_groups;
    if (pack_multi_check(table_host, n_entries, total_groups) != VITAE_OK) return 0;
    return cdiv(total_groups, (long)PACK_GROUPS);
}

extern "C" int vitae_conv3d_pack_multi_chunk_list(const long long* table_host, long n_entries, int* chunks_host, long n_chunks) {
    long total_groups;
    if (const int rc = pack_multi_check(table_host, n_entries, total_groups)) return rc;
    if (!chunks_host || n_chunks != cdiv(total_groups, (long)PACK_GROUPS)) return VITAE_ERR_INVALID_ARG;
    return pack_multi_walk(table_host, n_entries, n_chunks, chunks_host, nullptr) ? VITAE_OK : VITAE_ERR_INVALID_ARG;
}

extern "C" int vitae_conv3d_pack_weights_multi(const long long* table_host, const long long* table_dev, long n_entries, const int* chunks_host,
                                               const int* chunks_dev, long n_chunks, void* stream) {
    long total_groups;
    if (const int rc = pack_multi_check(table_host, n_entries, total_groups)) return rc;
    if (!table_dev || !chunks_host || !chunks_dev || n_chunks != cdiv(total_groups, (long)PACK_GROUPS)) return VITAE_ERR_INVALID_ARG;
    if (!pack_multi_walk(table_host, n_entries, n_chunks, nullptr, chunks_host)) return VITAE_ERR_INVALID_ARG;
    hipLaunchKernelGGL(conv3d_pack_multi_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const PackEntry*>(table_dev), (int)n_entries, chunks_dev, total_groups);
    return vitae_launch_status();
}

extern "C" int vitae_to_channels_last_bf16(const float* x, void* x16, int N, int C, int D, int H, int W, void* stream) {
    return run_channels_last(x, reinterpret_cast<__bf16*>(x16), N, C, D, H, W, stream);
}

extern "C" int vitae_to_channels_last_f32(const float* x, float* out, int N, int C, int D, int H, int W, void* stream) {
    return run_channels_last(x, out, N, C, D, H, W, stream);
}

extern "C" int vitae_conv3d_fwd(const void* x16, const void* w16, float* y, void* y_bf16, int N, int D, int H, int W, int Cin, int Cout, int kd,
                                int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream) {
    if (!x16 || !w16 || (!y && !y_bf16)) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (!aligned16({x16, w16, y, y_bf16})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    return run_gather<OpBf16, false>(g, x16, w16, y, y_bf16, 0, stream);
}

extern "C" int vitae_conv3d_fwd_x3(const float* x, const void* w16x2, float* y, void* y_bf16, int N, int D, int H, int W, int Cin, int Cout, int kd,
                                   int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream) {
    if (!x || !w16x2 || (!y && !y_bf16)) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (!aligned16({x, w16x2, y, y_bf16})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    return run_gather<OpX3, false>(g, x, w16x2, y, y_bf16, 0, stream);
}

extern "C" int vitae_conv3d_bwd_input(const void* dy16, const void* w16t, float* dx, void* dx_bf16, int accumulate, int N, int D, int H, int W,
                                      int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream) {
    if (!dy16 || !w16t || (!dx && !dx_bf16) || (accumulate && !dx)) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (!aligned16({dy16, w16t, dx, dx_bf16})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    return run_gather<OpBf16, true>(g, dy16, w16t, dx, dx_bf16, accumulate, stream);
}

extern "C" int vitae_conv3d_bwd_input_x3(const float* dy, const void* w16x2t, float* dx, void* dx_bf16, int accumulate, int N, int D, int H, int W,
                                         int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream) {
    if (!dy || !w16x2t || (!dx && !dx_bf16) || (accumulate && !dx)) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (!aligned16({dy, w16x2t, dx, dx_bf16})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    return run_gather<OpX3, true>(g, dy, w16x2t, dx, dx_bf16, accumulate, stream);
}

extern "C" long vitae_conv3d_wgrad_ws_floats(int N, int D, int H, int W, int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd,
                                             int ph, int pw) {
    ConvGeo g;
    if (conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return 0;
    return (long)cdiv(g.M, WCHUNK) * Cout * g.K;
}

extern "C" int vitae_conv3d_bwd_weight(const void* dy16, const void* x16, float* dw, float* ws, long ws_floats, int accumulate, int N, int D, int H,
                                       int W, int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw,
                                       void* stream) {
    if (!dy16 || !x16 || !dw || !ws) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    int chunks;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (const int rc = wgrad_chunks(g, ws_floats, chunks)) return rc;
    return run_wgrad<OpBf16>(g, chunks, dy16, x16, dw, ws, accumulate, stream);
}

extern "C" int vitae_conv3d_bwd_weight_x3(const float* dy, const float* x, float* dw, float* ws, long ws_floats, int accumulate, int N, int D, int H,
                                          int W, int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw,
                                          void* stream) {
    if (!dy || !x || !dw || !ws) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    int chunks;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (const int rc = wgrad_chunks(g, ws_floats, chunks)) return rc;
    if (!aligned16({dy, x, dw, ws})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    return run_wgrad<OpX3>(g, chunks, dy, x, dw, ws, accumulate, stream);
}

extern "C" int vitae_maxpool3d_fwd(const float* x, float* y, void* y_bf16, void* idx, int N, int D, int H, int W, int C, void* stream) {
    if (!x || (!y && !y_bf16) || !idx) return VITAE_ERR_INVALID_ARG;
    int Do, Ho, Wo;
    long in_total, out_total;
    if (const int rc = pool_geo(N, D, H, W, C, Do, Ho, Wo, in_total, out_total)) return rc;
    hipLaunchKernelGGL(maxpool3d_fwd_kernel, dim3(cdiv(out_total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, reinterpret_cast<__bf16*>(y_bf16),
                       reinterpret_cast<unsigned char*>(idx), D, H, W, C, Do, Ho, Wo, out_total);
    return vitae_launch_status();
}

extern "C" int vitae_maxpool3d_bwd(const float* dy, const void* idx, float* dx, void* dx_bf16, int N, int D, int H, int W, int C, void* stream) {
    if (!dy || !idx || (!dx && !dx_bf16)) return VITAE_ERR_INVALID_ARG;
    int Do, Ho, Wo;
    long in_total, out_total;
    if (const int rc = pool_geo(N, D, H, W, C, Do, Ho, Wo, in_total, out_total)) return rc;
    hipLaunchKernelGGL(maxpool3d_bwd_kernel, dim3(cdiv(in_total, 256)), dim3(256), 0, (hipStream_t)stream, dy,
                       reinterpret_cast<const unsigned char*>(idx), dx, reinterpret_cast<__bf16*>(dx_bf16), D, H, W, C, Do, Ho, Wo, in_total);
    return vitae_launch_status();
}

extern "C" int vitae_rows_mean_fwd(const float* x, float* y, void* y_bf16, int N, int S, int C, void* stream) {
    if (!x || (!y && !y_bf16) || N <= 0 || S <= 0 || C <= 0) return VITAE_ERR_INVALID_ARG;
    const long total = (long)N * C;
    hipLaunchKernelGGL(rows_mean_fwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, reinterpret_cast<__bf16*>(y_bf16), S, C,
                       total);
    return vitae_launch_status();
}

extern "C" int vitae_rows_mean_bwd(const float* dy, float* dx, void* dx_bf16, int N, int S, int C, void* stream) {
    if (!dy || (!dx && !dx_bf16) || N <= 0 || S <= 0 || C <= 0) return VITAE_ERR_INVALID_ARG;
    const long total = (long)N * S * C;
    if (total > (long)INT_MAX * 128) return VITAE_ERR_UNSUPPORTED_SHAPE;
    hipLaunchKernelGGL(rows_mean_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, dy, dx, reinterpret_cast<__bf16*>(dx_bf16), S, C,
                       total);
    return vitae_launch_status();
}
