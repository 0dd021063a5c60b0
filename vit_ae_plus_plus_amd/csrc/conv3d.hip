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
// Safety: a gather is issued only under its predicate (row in range, k < K, source voxel inside the volume), so no address outside
// an operand is formed; offsets are 64-bit.  No LDS beyond a 343-entry tap table / a 64-row coordinate table.
#include "conv3d.hpp"

namespace {

// ------------------------------------------------------------------ packing
__global__ __launch_bounds__(256) void conv3d_pack_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int Cout, int Cin, int taps,
                                                          int Kp, int transposed, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int row = (int)(i / Kp), k = (int)(i % Kp);
    const int inner = transposed ? Cout : Cin;          // k = tap * inner + c
    float v = 0.f;
    if (k < taps * inner) {
        const int tap = k / inner, c = k % inner;
        const int co = transposed ? c : row, ci = transposed ? row : c;
        v = w[((long)co * Cin + ci) * taps + tap];
    }
    out[i] = (__bf16)v;
}

// Every operand of a network in one launch: the destinations laid end to end and cut into chunks of PACK_CHUNK elements; chunks[2 c],
// chunks[2 c + 1] = the entry in which chunk c begins and the offset there in groups of 8.  A thread converts 8 consecutive k of one
// row (a packed size is a multiple of 16, so a group lies in one row of one entry) with conv3d_pack_kernel's expression per element
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
        const int Cout = (int)e.Cout, Cin = (int)e.Cin;
        const int inner = tr ? Cout : Cin;                // k = tap * inner + c
        bf16x8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            float v = 0.f;
            if (k < taps * inner) {
                const int tap = k / inner, c = k % inner;
                const int co = tr ? c : row, ci = tr ? row : c;
                v = e.w[((long)co * Cin + ci) * taps + tap];
            }
            h[j] = lo ? (__bf16)(v - (float)(__bf16)v) : (__bf16)v;
        }
        *reinterpret_cast<bf16x8*>(e.out + o) = h;
    }
}

__global__ __launch_bounds__(256) void channels_last_bf16_kernel(const float* __restrict__ x, __bf16* __restrict__ out, int C, long S, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;      // output index: (n S + s) C + c
    if (i >= total) return;
    const int c = (int)(i % C);
    const long ns = i / C, n = ns / S, s = ns % S;
    out[i] = (__bf16)x[(n * C + c) * S + s];
}

// ------------------------------------------------------------------ forward / input gradient: one gather-GEMM
struct GatherArgs {
    const __bf16* src; const __bf16* wpk; float* out; __bf16* out16;
    int Ds, Hs, Ws, Cs;         // source volume of one sample, its channels
    int Dr, Hr, Wr;             // row space of one sample
    int M, Nout;                // rows, output columns
    int kd, kh, kw, sd, sh, sw, pd, ph, pw;
    int K, Kp, cs_shift;        // K = taps * Cs; Kp = K padded to the k step; log2(Cs) or -1
    int accum;                  // != 0: the result is added to what `out` holds
};

template <int G, bool BWD>
__global__ __launch_bounds__(256) void conv3d_gather_kernel(const GatherArgs a) {
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
    const __bf16* wrow = a.wpk + (long)(cok ? co : 0) * a.Kp + 8 * hi;
    const long nbase = (long)n * a.Ds;

    f32x16 acc;
    double tot[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; tot[i] = 0.; }
    int chain = 0;
    for (int k0 = 0; k0 < a.Kp; k0 += KSTEP) {
        bf16x8 av, bv;
#pragma unroll
        for (int j = 0; j < 8; ++j) { av[j] = (__bf16)0.f; bv[j] = (__bf16)0.f; }
        if (cok) bv = *reinterpret_cast<const bf16x8*>(wrow + k0);
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
            const __bf16* p = a.src + (((nbase + d) * a.Hs + h) * a.Ws + w) * a.Cs + ci;
            if (G == 8) av = *reinterpret_cast<const bf16x8*>(p);
            else if (G == 4) {
                const bf16x4 q = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
                for (int e = 0; e < 4; ++e) av[4 * g + e] = q[e];
            } else av[g] = *p;
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
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
void launch_gather(const GatherArgs& a, hipStream_t st) {
    const dim3 grid(cdiv(a.M, 128), cdiv(a.Nout, 32));
    if (a.Cs % 8 == 0) hipLaunchKernelGGL((conv3d_gather_kernel<8, BWD>), grid, dim3(256), 0, st, a);
    else if (a.Cs % 4 == 0) hipLaunchKernelGGL((conv3d_gather_kernel<4, BWD>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((conv3d_gather_kernel<1, BWD>), grid, dim3(256), 0, st, a);
}

// ------------------------------------------------------------------ weight gradient
// Workgroup = (128 k-columns: 32 per wave) x (32 output channels) x (one chunk of rows).  MFMA: A[row = co][k = m] = dy16[m, co],
// B[k = m][col = kcol] = x16[src(m, tap(kcol)), ci(kcol)].  The 8 rows of a lane's fragments are the same for the 32 lanes of a
// half wave; their decoded coordinates come from a 64-row table in LDS that the first wave refills every 64 rows.
__global__ __launch_bounds__(256) void conv3d_wgrad_part_kernel(const __bf16* __restrict__ dy16, const __bf16* __restrict__ x16,
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
            bf16x8 av, bv;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int ml = ks * KSTEP + 8 * hi + j;
                const int4 e = rowtab[ml];
                const bool rok = e.x >= 0;
                av[j] = (__bf16)0.f; bv[j] = (__bf16)0.f;
                if (rok && cok) av[j] = dy16[(long)(mb + ml) * g.Cout + co];
                const int d = e.y + tkd, h = e.z + tkh, w = e.w + tkw;
                if (rok && kok && d >= 0 && d < g.D && h >= 0 && h < g.H && w >= 0 && w < g.W)
                    bv[j] = x16[((((long)e.x * g.D + d) * g.H + h) * g.W + w) * g.Cin + ci];
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
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

GatherArgs gather_args(const ConvGeo& g, bool bwd, const void* src, const void* wpk, float* out, void* out16) {
    GatherArgs a;
    a.src = reinterpret_cast<const __bf16*>(src); a.wpk = reinterpret_cast<const __bf16*>(wpk);
    a.out = out; a.out16 = reinterpret_cast<__bf16*>(out16);
    if (!bwd) { a.Ds = g.D; a.Hs = g.H; a.Ws = g.W; a.Cs = g.Cin; a.Dr = g.Do; a.Hr = g.Ho; a.Wr = g.Wo; a.M = (int)g.M; a.Nout = g.Cout; }
    else { a.Ds = g.Do; a.Hs = g.Ho; a.Ws = g.Wo; a.Cs = g.Cout; a.Dr = g.D; a.Hr = g.H; a.Wr = g.W; a.M = (int)g.V; a.Nout = g.Cin; }
    a.kd = g.kd; a.kh = g.kh; a.kw = g.kw; a.sd = g.sd; a.sh = g.sh; a.sw = g.sw; a.pd = g.pd; a.ph = g.ph; a.pw = g.pw;
    a.K = g.taps * a.Cs; a.Kp = (int)kpad(a.K); a.cs_shift = shift_of(a.Cs); a.accum = 0;
    return a;
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
    if (!w || !w16 || Cout <= 0 || Cin <= 0) return VITAE_ERR_INVALID_ARG;
    if (kd < 1 || kh < 1 || kw < 1 || kd > 7 || kh > 7 || kw > 7 || (Cout & 3)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const int taps = kd * kh * kw;
    const long Kp = kpad((long)taps * (transposed ? Cout : Cin));
    if (Kp > (long)INT_MAX - 256) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const long total = (long)(transposed ? Cin : Cout) * Kp;
    hipLaunchKernelGGL(conv3d_pack_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w, reinterpret_cast<__bf16*>(w16), Cout, Cin,
                       taps, (int)Kp, transposed ? 1 : 0, total);
    return vitae_launch_status();
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
    if (!x || !x16 || N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return VITAE_ERR_INVALID_ARG;
    const long S = (long)D * H * W, total = (long)N * S * C;
    if (total > (long)INT_MAX * 128) return VITAE_ERR_UNSUPPORTED_SHAPE;
    hipLaunchKernelGGL(channels_last_bf16_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, reinterpret_cast<__bf16*>(x16), C, S,
                       total);
    return vitae_launch_status();
}

extern "C" int vitae_conv3d_fwd(const void* x16, const void* w16, float* y, void* y_bf16, int N, int D, int H, int W, int Cin, int Cout, int kd,
                                int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream) {
    if (!x16 || !w16 || (!y && !y_bf16)) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (!aligned16({x16, w16, y, y_bf16})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    launch_gather<false>(gather_args(g, false, x16, w16, y, y_bf16), (hipStream_t)stream);
    return vitae_launch_status();
}

extern "C" int vitae_conv3d_bwd_input(const void* dy16, const void* w16t, float* dx, void* dx_bf16, int accumulate, int N, int D, int H, int W,
                                      int Cin, int Cout, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph, int pw, void* stream) {
    if (!dy16 || !w16t || (!dx && !dx_bf16) || (accumulate && !dx)) return VITAE_ERR_INVALID_ARG;
    ConvGeo g;
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    if (!aligned16({dy16, w16t, dx, dx_bf16})) return VITAE_ERR_UNSUPPORTED_SHAPE;
    GatherArgs a = gather_args(g, true, dy16, w16t, dx, dx_bf16);
    a.accum = accumulate ? 1 : 0;
    launch_gather<true>(a, (hipStream_t)stream);
    return vitae_launch_status();
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
    if (const int rc = conv_geo(g, N, D, H, W, Cin, Cout, kd, kh, kw, sd, sh, sw, pd, ph, pw)) return rc;
    const int chunks = cdiv(g.M, WCHUNK);
    if (ws_floats < (long)chunks * Cout * g.K) return VITAE_ERR_INVALID_ARG;
    if (chunks > 65535) return VITAE_ERR_UNSUPPORTED_SHAPE;                     // grid.z
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(conv3d_wgrad_part_kernel, dim3(cdiv(g.K, 128), cdiv(Cout, 32), chunks), dim3(256), 0, st,
                       reinterpret_cast<const __bf16*>(dy16), reinterpret_cast<const __bf16*>(x16), ws, g);
    const long total = (long)Cout * g.K;
    hipLaunchKernelGGL(conv3d_wgrad_sum_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, ws, dw, chunks, Cout, Cin, g.taps, accumulate ? 1 : 0);
    return vitae_launch_status();
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
