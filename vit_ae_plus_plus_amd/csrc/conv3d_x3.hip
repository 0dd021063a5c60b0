// The fp32x3 route of the 3-D ResNet: the gather-GEMMs of conv3d.hip with fp32 sources and split operands.
//
// Every fp32 value v enters the bf16 MFMA as two halves, hi = bf16(v) and lo = bf16(v - float(hi)), so v is carried to ~2^-16
// relative instead of 2^-8.  A product is formed as three terms into ONE accumulator, in this fixed order per k-step:
//
//     acc = mfma(a_lo, b_hi, acc);   acc = mfma(a_hi, b_lo, acc);   acc = mfma(a_hi, b_hi, acc);      (cross terms first, then hi.hi)
//
// lo.lo (<= 2^-16 of the product) is dropped.  a = the gathered row operand: the route's fp32 channels-last activation or
// gradient, split in registers by the lane that gathered it — no producer writes extra planes.  b = the weight, packed once per
// optimiser step as two bf16 planes per row, [hi (Kp) | lo (Kp)], in conv3d.hip's k = tap * inner + c order with zero tails.  The
// weight gradient splits both of its fp32 operands (dy, x) in registers.  Everything else is conv3d.hip's: the operand maps of
// v_mfma_f32_32x32x16_bf16, the two-level accumulation (fp32 chains of FLUSH k-steps — now 3 FLUSH MFMAs — added to a double
// total), the chunked weight gradient with its ordered double sum, no float atomics.
//
// Gather widths follow the source's channel count: 32 bytes (two 16-byte loads of consecutive addresses) when Cs % 8 == 0, 16
// bytes when Cs % 4 == 0, element by element otherwise (the 1-channel stem).
//
// Safety: a gather is issued only under its predicate (row in range, k < K, source voxel inside the volume), so no address outside
// an operand is formed; offsets are 64-bit.  A non-finite source gives a NaN lo half (inf - inf), so it poisons what reads it.
#include "conv3d.hpp"

namespace {

__device__ __forceinline__ void split(float v, __bf16& hi, __bf16& lo) {
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);
}

__device__ __forceinline__ f32x16 mfma_x3(const bf16x8& ahi, const bf16x8& alo, const bf16x8& bhi, const bf16x8& blo, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alo, bhi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, blo, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahi, bhi, acc, 0, 0, 0);
}

// ------------------------------------------------------------------ packing: [rows][hi (Kp) | lo (Kp)]
__global__ __launch_bounds__(256) void conv3d_pack_x3_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int Cout, int Cin, int taps,
                                                             int Kp, int transposed, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;              // over [row][k] of ONE plane; both planes are written here
    if (i >= total) return;
    const int row = (int)(i / Kp), k = (int)(i % Kp);
    const int inner = transposed ? Cout : Cin;          // k = tap * inner + c
    float v = 0.f;
    if (k < taps * inner) {
        const int tap = k / inner, c = k % inner;
        const int co = transposed ? c : row, ci = transposed ? row : c;
        v = w[((long)co * Cin + ci) * taps + tap];
    }
    __bf16 hi, lo;
    split(v, hi, lo);
    out[2L * row * Kp + k] = hi;
    out[2L * row * Kp + Kp + k] = lo;
}

__global__ __launch_bounds__(256) void channels_last_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int C, long S, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;      // output index: (n S + s) C + c
    if (i >= total) return;
    const int c = (int)(i % C);
    const long ns = i / C, n = ns / S, s = ns % S;
    out[i] = x[(n * C + c) * S + s];
}

// ------------------------------------------------------------------ forward / input gradient: one gather-GEMM
struct GatherArgsX3 {
    const float* src; const __bf16* wpk; float* out; __bf16* out16;
    int Ds, Hs, Ws, Cs;         // source volume of one sample, its channels
    int Dr, Hr, Wr;             // row space of one sample
    int M, Nout;                // rows, output columns
    int kd, kh, kw, sd, sh, sw, pd, ph, pw;
    int K, Kp, cs_shift;        // K = taps * Cs; Kp = K padded to the k step (one plane of a packed row); log2(Cs) or -1
    int accum;                  // != 0: the result is added to what `out` holds
};

template <int G, bool BWD>
__global__ __launch_bounds__(256) void conv3d_gather_x3_kernel(const GatherArgsX3 a) {
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
    const __bf16* wrow = a.wpk + (long)(cok ? co : 0) * (2L * a.Kp) + 8 * hi;
    const long nbase = (long)n * a.Ds;

    f32x16 acc;
    double tot[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; tot[i] = 0.; }
    int chain = 0;
    for (int k0 = 0; k0 < a.Kp; k0 += KSTEP) {
        float v[8];
        bf16x8 ahi, alo, bhi, blo;
#pragma unroll
        for (int j = 0; j < 8; ++j) { v[j] = 0.f; bhi[j] = (__bf16)0.f; blo[j] = (__bf16)0.f; }
        if (cok) {
            bhi = *reinterpret_cast<const bf16x8*>(wrow + k0);
            blo = *reinterpret_cast<const bf16x8*>(wrow + a.Kp + k0);
        }
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
            const float* p = a.src + (((nbase + d) * a.Hs + h) * a.Ws + w) * a.Cs + ci;
            if (G == 8) {
                const f32x4 q0 = *reinterpret_cast<const f32x4*>(p), q1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[e] = q0[e]; v[4 + e] = q1[e]; }
            } else if (G == 4) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * g + e] = q[e];
            } else v[g] = *p;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 h_, l_;
            split(v[j], h_, l_);
            ahi[j] = h_; alo[j] = l_;
        }
        acc = mfma_x3(ahi, alo, bhi, blo, acc);
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

template <bool BWD>
void launch_gather_x3(const GatherArgsX3& a, hipStream_t st) {
    const dim3 grid(cdiv(a.M, 128), cdiv(a.Nout, 32));
    if (a.Cs % 8 == 0) hipLaunchKernelGGL((conv3d_gather_x3_kernel<8, BWD>), grid, dim3(256), 0, st, a);
    else if (a.Cs % 4 == 0) hipLaunchKernelGGL((conv3d_gather_x3_kernel<4, BWD>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv3d_gather_x3_kernel<1, BWD>), grid, dim3(256), 0, st, a);
}

GatherArgsX3 gather_args_x3(const ConvGeo& g, bool bwd, const float* src, const void* wpk, float* out, void* out16) {
    GatherArgsX3 a;
    a.src = src; a.wpk = reinterpret_cast<const __bf16*>(wpk);
    a.out = out; a.out16 = reinterpret_cast<__bf16*>(out16);
    if (!bwd) { a.Ds = g.D; a.Hs = g.H; a.Ws = g.W; a.Cs = g.Cin; a.Dr = g.Do; a.Hr = g.Ho; a.Wr = g.Wo; a.M = (int)g.M; a.Nout = g.Cout; }
    else { a.Ds = g.Do; a.Hs = g.Ho; a.Ws = g.Wo; a.Cs = g.Cout; a.Dr = g.D; a.Hr = g.H; a.Wr = g.W; a.M = (int)g.V; a.Nout = g.Cin; }
    a.kd = g.kd; a.kh = g.kh; a.kw = g.kw; a.sd = g.sd; a.sh = g.sh; a.sw = g.sw; a.pd = g.pd; a.ph = g.ph; a.pw = g.pw;
    a.K = g.taps * a.Cs; a.Kp = (int)kpad(a.K); a.cs_shift = shift_of(a.Cs); a.accum = 0;
    return a;
}

// ------------------------------------------------------------------ weight gradient
// conv3d_wgrad_part_kernel with fp32 operands: A[row = co][k = m] = dy[m, co], B[k = m][col = kcol] = x[src(m, tap(kcol)), ci(kcol)],
// both split in registers.  Same workgroup shape, row table, chunking and flush points.
__global__ __launch_bounds__(256) void conv3d_wgrad_part_x3_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ ws,
                                                                   const ConvGeo g) {
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
            bf16x8 ahi, alo, bhi, blo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ml = ks * KSTEP + 8 * hi + j;
                const int4 e = rowtab[ml];
                const bool rok = e.x >= 0;
                float av = 0.f, bv = 0.f;
                if (rok && cok) av = dy[(long)(mb + ml) * g.Cout + co];
                const int d = e.y + tkd, h = e.z + tkh, w = e.w + tkw;
                if (rok && kok && d >= 0 && d < g.D && h >= 0 && h < g.H && w >= 0 && w < g.W)
                    bv = x[((((long)e.x * g.D + d) * g.H + h) * g.W + w) * g.Cin + ci];
                __bf16 h_, l_;
                split(av, h_, l_); ahi[j] = h_; alo[j] = l_;
                split(bv, h_, l_); bhi[j] = h_; blo[j] = l_;
            }
            acc = mfma_x3(ahi, alo, bhi, blo, acc);
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

}  // namespace

extern "C" long vitae_conv3d_packed_elems_x3(int Cout, int Cin, int kd, int kh, int kw, int transposed) {
    return 2 * vitae_conv3d_packed_elems(Cout, Cin, kd, kh, kw, transposed);
}

extern "C" int vitae_conv3d_pack_weight_x3(const float* w, void* w16x2, int Cout, int Cin, int kd, int kh, int kw, int transposed, void* stream) {
    if (!w || !w16x2 || Cout <= 0 || Cin <= 0) return VITAE_ERR_INVALID_ARG;
    if (kd < 1 || kh < 1 || kw < 1 || kd > 7 || kh > 7 || kw > 7 || (Cout & 3)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const int taps = kd * kh * kw;
    const long Kp = kpad((long)taps * (transposed ? Cout : Cin));
    if (Kp > (long)INT_MAX - 256 || ((uintptr_t)w16x2 & 15)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const long total = (long)(transposed ? Cin : Cout) * Kp;
    hipLaunchKernelGGL(conv3d_pack_x3_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, reinterpret_cast<__bf16*>(w16x2), Cout,
                       Cin, taps, (int)Kp, transposed ? 1 : 0, total);
    return vitae_launch_status();
}

extern "C" int vitae_to_channels_last_f32(const float* x, float* out, int N, int C, int D, int H, int W, void* stream) {
    if (!x || !out || N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return VITAE_ERR_INVALID_ARG;
    const long S = (long)D * H * W, total = (long)N * S * C;
    if (total > (long)INT_MAX * 128) return VITAE_ERR_UNSUPPORTED_SHAPE;
    hipLaunchKernelGGL(channels_last_f32_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, out, C, S, total);
    return vitae_launch_status();
}

extern "C" int vitae_conv3d_fwd_x3(const float* x, const void* w16x2, float* y, void* y_bf16, int N, int D, int H, int W, int Cin, int Cout, int kd,
                                   int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream) {
    if (!x || !w16x2 || (!y && !y_bf16)) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (!aligned16({x, w16x2, y, y_bf16})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    launch_gather_x3<false>(gather_args_x3(g, false, x, w16x2, y, y_bf16), (hipStream_t)stream);
    return vitae_launch_status();
}

extern "C" int vitae_conv3d_bwd_input_x3(const float* dy, const void* w16x2t, float* dx, void* dx_bf16, int accumulate, int N, int D, int H, int W,
                                         int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream) {
    if (!dy || !w16x2t || (!dx && !dx_bf16) || (accumulate && !dx)) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (!aligned16({dy, w16x2t, dx, dx_bf16})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    GatherArgsX3 a = gather_args_x3(g, true, dy, w16x2t, dx, dx_bf16);
    a.accum = accumulate ? 1 : 0;
    launch_gather_x3<true>(a, (hipStream_t)stream);
    return vitae_launch_status();
}

extern "C" int vitae_conv3d_bwd_weight_x3(const float* dy, const float* x, float* dw, float* ws, long ws_floats, int accumulate, int N, int D, int H,
                                          int W, int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw,
                                          void* stream) {
    if (!dy || !x || !dw || !ws) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    const int chunks = cdiv(g.M, WCHUNK);
    if (ws_floats < (long)chunks * Cout * g.K) return VITAE_ERR_INVALID_ARG;
    if (chunks > 65535) return VITAE_ERR_UNSUPPORTED_SHAPE;                     // grid.z
    if (!aligned16({dy, x, dw, ws})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv3d_wgrad_part_x3_kernel, dim3(cdiv(g.K, 128), cdiv(Cout, 32), chunks), dim3(256), 0, st, dy, x, ws, g);
    const long total = (long)Cout * g.K;
    hipLaunchKernelGGL(conv3d_wgrad_sum_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, ws, dw, chunks, Cout, Cin, g.taps, accumulate ? 1 : 0);
    return vitae_launch_status();
}
