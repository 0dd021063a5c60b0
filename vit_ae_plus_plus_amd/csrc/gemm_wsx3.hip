// fp32x3 on the wave-specialised 64 x 64 workgroup of gemm_ws64.hip (round 4; the consumers' k-loop is the shared ws64_consume of
// gemm_bt.hpp, their tail a copy of gemm_ws64_body's without the stamps).
// The fp32-grade fast mode multiplies fp32 operands as bf16 hi + lo pairs (hi.hi + hi.lo + lo.hi, fp32 accumulate).  Here the
// PRODUCER waves — idle VALUs — do the split: they load the fp32 operand tiles with ordinary 16-byte loads (two k-tiles ahead,
// in registers), form hi = bf16(x), lo = bf16(x - hi) and write both images into LDS in exactly the layout the LDS-DMA leaves
// (same source permutation, same fragment reads).  Nothing upstream changes: every producer of an fp32 activation stays as it is.
// A stage = [A hi | B hi | A lo | B lo] = 32 KB; the look-ahead lives in registers, so TWO stages suffice (64 KB: two workgroups
// per CU).  The reduction length is any multiple of 4 (token counts are not padded on the fp32 side): the tail is zero-filled.
#include "gemm_bt.hpp"

namespace vglds {

#ifndef VITAE_X3_PRODUCERS
#define VITAE_X3_PRODUCERS 4      // producer waves of the fp32x3 workgroup (8: half the conversion work per wave, one workgroup per CU)
#endif
// The loads are UNCONDITIONAL (clamped addresses) and the zero-fill of the reduction's tail is applied when the values are
// converted: a load behind a condition — or a select right behind it — makes hipcc wait for every load in flight (vmcnt(0)), which
// exposed a full memory latency per k-tile (0.78 us per tile instead of 0.35).
// ... and they are INLINE ASM: hipcc's own vmcnt bookkeeping across the loop's back edge waited for the younger register set too
// (vmcnt(7) .. vmcnt(0) in front of the older set's conversion), so a tile's loads had half a k-tile of flight time.  The caller
// counts: 8 loads per wave and tile, `wait_vmcnt<8>` in front of a conversion while the other set is in flight, then x3_tie.
__device__ __forceinline__ f32x4 x3_ld(const float* ptr) {
    f32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(r) : "v"(ptr) : "memory");
    return r;
}
__device__ __forceinline__ void x3_tie(f32x4& v) { asm volatile("" : "+v"(v)); }

template <int ROWS, bool KC>
__device__ __forceinline__ void x3_load_piece(const float* __restrict__ P, long ld, int rows, int K, int r0, int k0, int pw, int lane, int j,
                                              f32x4 (&v)[2]) {
    constexpr int LINE_CH = KC ? BK / 8 : ROWS / 8, LPI = 64 / LINE_CH, NI = pieces<ROWS, KC, VITAE_X3_PRODUCERS>();
    const int inst = pw * NI + j;
    const int line = inst * LPI + lane / LINE_CH;
    const int slot = lane % LINE_CH;
    const int chunk = slot ^ swz<KC, LINE_CH>(line);
    if (KC) {
        const int gr = min(r0 + line, rows - 1);
        const int k = k0 + chunk * 8;
        const float* src = P + (long)gr * ld;
        v[0] = x3_ld(src + min(k, K - 4));
        v[1] = x3_ld(src + min(k + 4, K - 4));
    } else {
        // rows are a multiple of 4 only (fp32 activations are not padded): each 4-row group clamped on its own — groups past
        // the operand read a valid group and are never stored
        const int g0 = min(r0 + chunk * 8, rows - 4), g1 = min(r0 + chunk * 8 + 4, rows - 4);
        const float* src = P + (long)min(k0 + line, K - 1) * ld;
        v[0] = x3_ld(src + g0);
        v[1] = x3_ld(src + g1);
    }
}
template <int ROWS, bool KC>
__device__ __forceinline__ void x3_store_piece(const f32x4 (&v)[2], int K, int k0, bool full, unsigned char* hi_img, unsigned char* lo_img, int pw, int lane, int j) {
    constexpr int LINE_CH = KC ? BK / 8 : ROWS / 8, LPI = 64 / LINE_CH, NI = pieces<ROWS, KC, VITAE_X3_PRODUCERS>();
    const int inst = pw * NI + j;
    const int line = inst * LPI + lane / LINE_CH;
    const int chunk = (lane % LINE_CH) ^ swz<KC, LINE_CH>(line);
    // which of the two 4-element groups lie inside the reduction (K % 4 == 0)
    const int k = KC ? k0 + chunk * 8 : k0 + line;
    const bool in0 = k < K, in1 = KC ? k + 4 < K : k < K;
    // 24 VALU operations per 8 elements (the naive form compiled to 40, and the producers' conversion was the k-loop's bound):
    // pairs converted once (v_cvt_pk_bf16_f32), the two hi values of a pair taken back out of the packed word by a shift / a mask
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 h, l;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float x0 = v[q >> 1][2 * (q & 1)], x1 = v[q >> 1][2 * (q & 1) + 1];
        if (!full) {
            const bool in = (q >> 1) ? in1 : in0;
            x0 = in ? x0 : 0.f; x1 = in ? x1 : 0.f;
        }
        const unsigned ph = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
        const float h0 = __builtin_bit_cast(float, ph << 16), h1 = __builtin_bit_cast(float, ph & 0xffff0000u);
        h[q] = ph;
        l[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0 - h0, x1 - h1}, bf16x2));
    }
    *reinterpret_cast<u32x4*>(hi_img + inst * 1024 + lane * 16) = h;
    *reinterpret_cast<u32x4*>(lo_img + inst * 1024 + lane * 16) = l;
}

template <bool A_KC, bool B_KC, bool RS>
__device__ __forceinline__ void gemm_wsx3_body(const GArgs& p, const WsHot& h, const int bid, const int zid, unsigned char* smem) {
    constexpr int BM = 64, BN = 64, NWC = 4;
    constexpr int IMG = 64 * BK * 2, STG = 4 * IMG;                      // [A hi | B hi | A lo | B lo]
    constexpr int PA = pieces<BM, A_KC, VITAE_X3_PRODUCERS>(), PB = pieces<BN, B_KC, VITAE_X3_PRODUCERS>();
    const float* Af = reinterpret_cast<const float*>(h.A);
    const float* Bf = reinterpret_cast<const float*>(h.B);
    // the XCD-balanced tile map (gemm_bt.hpp)
    const int T = h.tiles_m * h.tiles_n;
    const int xq = T >> 3, xr = T & 7, xcd = bid & 7;
    const int lin = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
    if ((bid >> 3) >= xq + (xcd < xr ? 1 : 0)) return;
    const int tn = (h.xcd_m & 1) ? lin % h.tiles_n : lin / h.tiles_m;
    const int tm = (h.xcd_m & 1) ? lin / h.tiles_n : lin % h.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = zid * h.kps;
    const int kend = min(h.K, kbeg + h.kps);
    const int nk = (kend - kbeg + BK - 1) / BK;                          // >= 1; the last tile may be partly past kend (zero-filled)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= NWC) {
        // ---------------- producers: fp32 loads two tiles ahead, split, LDS writes ----------------
        const int pw = wave - NWC;
        f32x4 ra[2][PA][2], rb[2][PB][2];
        auto load = [&](int t, auto set_c) {
            constexpr int SET = decltype(set_c)::value;
            const int k0 = kbeg + t * BK;
#pragma unroll
            for (int j = 0; j < PA; ++j) x3_load_piece<BM, A_KC>(Af, h.lda, h.M, kend, m0, k0, pw, lane, j, ra[SET][j]);
#pragma unroll
            for (int j = 0; j < PB; ++j) x3_load_piece<BN, B_KC>(Bf, h.ldb, h.N, kend, n0, k0, pw, lane, j, rb[SET][j]);
        };
        auto store = [&](int t, int stage, auto set_c, bool other_in_flight) {
            constexpr int SET = decltype(set_c)::value;
            unsigned char* st = smem + stage * STG;
            const int k0 = kbeg + t * BK;
            if (other_in_flight) wait_vmcnt<PA * 2 + PB * 2>(); else wait_vmcnt<0>();
#pragma unroll
            for (int j = 0; j < PA; ++j) { x3_tie(ra[SET][j][0]); x3_tie(ra[SET][j][1]); }
#pragma unroll
            for (int j = 0; j < PB; ++j) { x3_tie(rb[SET][j][0]); x3_tie(rb[SET][j][1]); }
            const bool full = k0 + BK <= kend;          // wave-uniform: only the last tile of a ragged reduction masks
#pragma unroll
            for (int j = 0; j < PA; ++j) x3_store_piece<BM, A_KC>(ra[SET][j], kend, k0, full, st, st + 2 * IMG, pw, lane, j);
#pragma unroll
            for (int j = 0; j < PB; ++j) x3_store_piece<BN, B_KC>(rb[SET][j], kend, k0, full, st + IMG, st + 3 * IMG, pw, lane, j);
        };
        using S0 = std::integral_constant<int, 0>; using S1 = std::integral_constant<int, 1>;
        load(0, S0{});
        if (nk > 1) load(1, S1{});
        // tile t goes into stage t & 1 after B_{t-1} (every read of tile t - 2 retired before it); B_t publishes it
#pragma unroll 1
        for (int t = 0; t < nk; t += 2) {
            store(t, 0, S0{}, t + 1 < nk);
            if (t + 2 < nk) load(t + 2, S0{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            wg_barrier();                                                // B_t
            if (t + 1 < nk) {
                store(t + 1, 1, S1{}, t + 2 < nk);
                if (t + 3 < nk) load(t + 3, S1{});
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                wg_barrier();                                            // B_{t+1}
            }
        }
        return;
    }
    // ---------------- consumers: hi / lo fragments, three MFMAs per pair ----------------
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, hi = lane >> 5;
    f32x16 acc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[h][i] = 0.f;
    const bool rowsum = RS && p.a_rowsum != nullptr && tn == 0 && wn == 0;
    f32x16 accx;
#pragma unroll
    for (int i = 0; i < 16; ++i) accx[i] = 0.f;
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;
    bf16x8 fah[BK / 16], fal[BK / 16], fbh[BK / 16], fbl[BK / 16];
    constexpr int RK = 2 * ((A_KC ? 1 : 2) + (B_KC ? 1 : 2));
    auto rd = [&](const unsigned char* ST, auto kk_c) {
        constexpr int kk = decltype(kk_c)::value;
        fah[kk] = frag_asm<BM, A_KC>(ST, wm * 32, kk, lane);
        fbh[kk] = frag_asm<BN, B_KC>(ST + IMG, wn * 32, kk, lane);
        fal[kk] = frag_asm<BM, A_KC>(ST + 2 * IMG, wm * 32, kk, lane);
        fbl[kk] = frag_asm<BN, B_KC>(ST + 3 * IMG, wn * 32, kk, lane);
    };
    auto mm = [&](auto kk_c) {
        constexpr int kk = decltype(kk_c)::value;
        frag_tie(fah[kk]); frag_tie(fbh[kk]); frag_tie(fal[kk]); frag_tie(fbl[kk]);
        // the two cross terms first: they are 2^-8 of the main term
        acc[kk & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal[kk], fbh[kk], acc[kk & 1], 0, 0, 0);
        acc[kk & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah[kk], fbl[kk], acc[kk & 1], 0, 0, 0);
        acc[kk & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah[kk], fbh[kk], acc[kk & 1], 0, 0, 0);
        if constexpr (RS) {
            if (rowsum) {
                accx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal[kk], ones, accx, 0, 0, 0);
                accx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fah[kk], ones, accx, 0, 0, 0);
            }
        }
    };
    const int nq = n0 + wn * 32 + 4 * (lane % 8);
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias && nq < p.N) bias4 = *reinterpret_cast<const f32x4*>(p.bias + nq);
    wg_barrier();                                                        // B_0
    ws64_consume<(2 * RK > 15 ? 15 : 2 * RK), 2, STG>(smem, nk, rd, mm);
    if (RS && rowsum && l31 == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + crow(r, hi);
            if (m < p.M) atomicAdd(p.a_rowsum + m, accx[r]);
        }
    }
    // the tail of gemm_ws64_body without its stamps (why it is a copy: see there)
    f32x16 accs[1][1];
#pragma unroll
    for (int i = 0; i < 16; ++i) accs[0][0][i] = acc[0][i] + acc[1][i];
    __syncthreads();                                                     // (consumers only: the producers have left) stages are free
    float* Tw = reinterpret_cast<float*>(smem) + wave * 1024;
    if (p.splits > 1) {
        const int tile = p.tile0 + tm * p.tiles_n + tn;
        float* part = p.ws + VITAE_GLDS_TICKETS + (long)tile * p.splits * (BM * BN);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(part, 0, p.splits * (BM * BN * 4), 0x00020000);
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const int toff = (int)threadIdx.x * 16;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 v = {accs[0][0][4 * g], accs[0][0][4 * g + 1], accs[0][0][4 * g + 2], accs[0][0][4 * g + 3]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (zid * 4 + g) * (256 * 16) + toff, 0, 16);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* flag = reinterpret_cast<int*>(smem + 4 * 4096);
        if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add(reinterpret_cast<int*>(p.ws) + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*flag != p.splits - 1) return;
#pragma unroll
        for (int i = 0; i < 16; ++i) accs[0][0][i] = 0.f;
#pragma unroll 1
        for (int sp0 = 0; sp0 < p.splits; sp0 += 4) {
            f32x4 v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int sp = min(sp0 + u, p.splits - 1);
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    v[u][g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (sp * 4 + g) * (256 * 16) + toff, 0, 16));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (sp0 + u < p.splits) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) accs[0][0][4 * g + e] += v[u][g][e];
                }
        }
        if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<int*>(p.ws) + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    bt_park_quadrant<1, 1, 1>(accs, lane, Tw);
    __builtin_amdgcn_wave_barrier();
    float sqs = 0.f;
    { f32x4 cz = {0.f, 0.f, 0.f, 0.f}; bt_wave_epilogue<1, 1>(p, bt_epilogue_kind(p), m0 + wm * 32, n0 + wn * 32, Tw, lane, sqs, bias4, cz, false); }
    if (p.sqacc) {
        sqs = wave_sum(sqs);
        float* red = reinterpret_cast<float*>(smem + 4 * 4096 + 64);
        if (lane == 0) red[wave] = sqs;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(sq_slot(p), (double)((red[0] + red[1]) + (red[2] + red[3])));
    }
}

template <bool A_KC, bool B_KC, bool RS>
__global__ __launch_bounds__(64 * (4 + VITAE_X3_PRODUCERS), VITAE_X3_PRODUCERS == 4 ? 4 : 3) void gemm_wsx3_kernel(WS_HOT_PARAMS, const GArgs p) {      // (4 producers: 4 waves per SIMD = <= 128 VGPRs, two workgroups per CU — the row-sum variant took 132)
    __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * 4 * 8192];      // the ONLY LDS object
    gemm_wsx3_body<A_KC, B_KC, RS>(p, WS_HOT_FROM_PARAMS, blockIdx.x, blockIdx.z, smem);
}

// resident workgroup slots of the chip for this kernel (the split-K rule fills about that many)
int wsx3_slots() { return VITAE_X3_PRODUCERS == 4 ? 512 : 256; }

// p: a complete descriptor with FLOAT operands behind p.A / p.B (vec_epi set); p.splits k-ranges, multiples of 64 except the last
int wsx3_launch(GArgs p, int a_kc, int b_kc, hipStream_t st) {
    if (!p.vec_epi || (p.K & 3) || p.splits < 1 || p.C16) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (!a_kc && b_kc) return VITAE_ERR_UNSUPPORTED_SHAPE;
    bt_k_ranges(p.K, 0, p.splits, p.k_per_split);                        // (any range length: the last k-tile is zero-filled)
    p.tiles_m = cdiv(p.M, 64); p.tiles_n = cdiv(p.N, 64); p.tile0 = 0;
    if (p.splits > 1 && (!p.ws || (long)p.tiles_m * p.tiles_n > VITAE_GLDS_TICKETS || p.epi == VITAE_EPI_GELU)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (p.a_rowsum && (a_kc || b_kc)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const dim3 grid(8 * cdiv((long)p.tiles_m * p.tiles_n, 8), 1, p.splits), block(64 * (4 + VITAE_X3_PRODUCERS));
    if (a_kc && b_kc) hipLaunchKernelGGL((gemm_wsx3_kernel<true, true, false>), grid, block, 0, st, WS_HOT_ARGS(p), p);
    else if (a_kc && !b_kc) hipLaunchKernelGGL((gemm_wsx3_kernel<true, false, false>), grid, block, 0, st, WS_HOT_ARGS(p), p);
    else if (p.a_rowsum) hipLaunchKernelGGL((gemm_wsx3_kernel<false, false, true>), grid, block, 0, st, WS_HOT_ARGS(p), p);
    else hipLaunchKernelGGL((gemm_wsx3_kernel<false, false, false>), grid, block, 0, st, WS_HOT_ARGS(p), p);
    return vitae_launch_status();
}

}  // namespace vglds
