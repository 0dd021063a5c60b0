// The wave-specialised structure of gemm_ws.hip (four MFMA waves, producer waves that only issue LDS-DMA, one workgroup barrier per
// k-tile) on a 64 x 64 tile (tile id 5): the few-row launches of the batch-4 / batch-8 step.  Stand-alone, with a two-plane weight
// operand, and as the paired dgrad + wgrad launch of one Linear's backward.
// At 440-1736 token rows a launch is 84-700 workgroups of a handful of k-tiles each, and a workgroup's k-step is a dependent
// chain (DMA issue, fragment reads, MFMAs, wait + barrier: ~610 clocks per 64-deep step in gemm_glds.hip, ~880 in its pipelined
// form inside the step).  With the roles split the chain is gone: a k-step costs what its 16 KB of operands cost the CU's
// L2 -> LDS path (~400 clocks).  Measured alone (us, ws64 / 64-row family / hipBLASLt): 440 x 2304 x 768 7.2 / 10.4 / 8.3,
// 440 x 768 x 768 6.5 / 8.4 / 7.2, 868 x 2048 x 512 7.8 / 9.7 / 9.4, weight-gradient form 2304 x 768 x 448 7.7 / 9.4.
// Each consumer wave owns ONE 32 x 32 fragment (two accumulators: even / odd k-slices).  80 KB of LDS and 97 VGPRs: two workgroups
// share a CU.  In-launch split-K as in the family (partials through write-through stores, ticket, last arriver sums in split
// order); RS: the consumer waves of column tile 0 add the row sums of A (one more MFMA against ones per k-slice) = the bias
// gradient colsum(dy) of a weight-gradient launch.
#include "gemm_bt.hpp"

namespace vglds {

#ifndef VITAE_WS64_STAGES
#define VITAE_WS64_STAGES 4         // 64 KB (the epilogue aliases the stages): TWO workgroups per CU, three k-tiles in flight each
#endif
constexpr int WS64_SMEM = VITAE_WS64_STAGES * 16384;
// W2 (round 5, forward form only): the B operand (a weight matrix) comes as TWO bf16 planes, hi = bf16(W) and lo = bf16(W - hi)
// (p.B / p.B2, same layout): a stage is [A | B hi | B lo] and every k-slice takes two MFMAs, x16 Wlo^T + x16 Whi^T — the weight
// enters at ~2^-17 instead of 2^-9 while the activations stay bf16.  Why: tools/bf16_rounding_ablation.py — the bf16 schedule's
// loss error against the fp32 reference is carried by the rounding of the WEIGHTS in the forward (1.3e-4 of 1.5e-4 on the total;
// activations 9e-6, the whole backward 4e-6), and the decoder's fc1 alone is 1.2e-4 of it.
// BM = 128 (tile id 7, round 7): the same workgroup on a 128 x 64 tile.  Each consumer wave owns TWO 32 x 32 fragments stacked along M
// (rows wm * 64 and wm * 64 + 32) that share one B fragment per k-slice; a stage is [A 16 KB | B 8 KB], three stages = 72 KB (the LDS
// geometry of the W2 form), 0.75x the LDS-fill bytes per flop and half the workgroups of the 64 x 64 tile.  ONE accumulator per
// fragment (the two fragments are the two independent MFMA chains): with the even / odd pair per fragment the weight-gradient form
// with row sums needs 64 + 48 (fragments of four k-slices) + 16 registers before any address — over the 128 of two workgroups per CU.
// So an output element is summed in k order, not in the 64 x 64 tile's even-then-odd order: equal to tile 5 to round-off, not bitwise.
// KINDS: the epilogue instantiations this body carries (gemm_bt.hpp, BT_KINDS_*).
// ROLE: 0 = the workgroup's waves split into producers and consumers here; 1 / 2 = the caller has split them already and this
// instantiation holds the producers' / the consumers' code only (gemm_ws64_pair_kernel: why is told there).
template <bool A_KC, bool B_KC, int S, bool RS, bool W2 = false, int BM = 64, int KINDS = BT_KINDS_ALL, int ROLE = 0>
__device__ __forceinline__ void gemm_ws64_body(const GArgs& p, const WsHot& h, const int bid, const int zid, unsigned char* smem) {
#ifndef VITAE_WS64_PRODUCERS
#define VITAE_WS64_PRODUCERS 4
#endif
    constexpr int BN = 64, NWC = 4, NWP = VITAE_WS64_PRODUCERS, FM = BM / 64;
    static_assert(BM == 64 || (BM == 128 && !W2), "64 or 128 rows");
    constexpr int A_T = BM * BK * 2, B_T = BN * BK * 2, STG = A_T + (W2 ? 2 : 1) * B_T;
    constexpr int PA = pieces<BM, A_KC, NWP>(), PB = pieces<BN, B_KC, NWP>(), PT = PA + (W2 ? 2 : 1) * PB;
    static_assert(!W2 || (A_KC && B_KC && !RS), "two weight planes: the forward form");
    static_assert(S >= 3 && S <= 5 && (S - 2) * PT <= 63, "stage count");
    // the XCD-balanced tile map (gemm_bt.hpp)
    const int T = h.tiles_m * h.tiles_n;
    const int xq = T >> 3, xr = T & 7, xcd = bid & 7;
    const int lin = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
    if ((bid >> 3) >= xq + (xcd < xr ? 1 : 0)) return;
    const int tn = (h.xcd_m & 1) ? lin % h.tiles_n : lin / h.tiles_m;
    const int tm = (h.xcd_m & 1) ? lin / h.tiles_n : lin % h.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = zid * h.kps;
    const int nk = (min(h.K, kbeg + h.kps) - kbeg) / BK;         // >= 2 (launcher)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tools/ws64_phase_probe.py: s_memtime stamps of consumer wave 0 (slots 0-7) and producer wave 4 (8-15) of every workgroup,
    // 16 per workgroup indexed by its position in the launch (blockIdx.x + gridDim.x * blockIdx.z)
    auto stamp = [&](int i) {
        if ((h.xcd_m & 2) && (threadIdx.x & 255) == 0) p.dbg[((long)blockIdx.z * gridDim.x + blockIdx.x) * 16 + i] = __builtin_amdgcn_s_memtime();
    };
    if (ROLE != 2 && (ROLE == 1 || wave >= NWC)) {
        // ---------------- producers ----------------
        const int pw = wave - NWC;
        stamp(8);
        auto issue_tile = [&](int t, int stage) {
            unsigned char* dst = smem + stage * STG;
            const int k0 = kbeg + t * BK;
#pragma unroll
            for (int j = 0; j < PA; ++j) dma_piece<BM, A_KC, NWP>(h.A, h.lda, h.M, m0, k0, dst, pw, lane, j);
#pragma unroll
            for (int j = 0; j < PB; ++j) dma_piece<BN, B_KC, NWP>(h.B, h.ldb, h.N, n0, k0, dst + A_T, pw, lane, j);
            if constexpr (W2) {
#pragma unroll
                for (int j = 0; j < PB; ++j) dma_piece<BN, B_KC, NWP>(h.B2, h.ldb, h.N, n0, k0, dst + A_T + B_T, pw, lane, j);
            }
        };
        const int npre = min(S - 1, nk);
        for (int t = 0; t < npre; ++t) issue_tile(t, t);
        stamp(9);                                                        // prologue issued
        wait_tiles<S, PT>(npre - 1);
        stamp(10);                                                       // first k-tile landed
        wg_barrier();                                                    // B_0
        int stage = npre % S;
#pragma unroll 1
        for (int t = 0; t + 1 < nk; ++t) {
            if (t + S - 1 < nk) {
                issue_tile(t + S - 1, stage);
                stage = stage + 1 == S ? 0 : stage + 1;
            }
            wait_tiles<S, PT>(min(t + S - 1, nk - 1) - (t + 1));
            wg_barrier();                                                // B_{t+1}
        }
        stamp(11);                                                       // last k-tile handed over
        return;
    }
    // ---------------- consumers ----------------
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, hi = lane >> 5;
    f32x16 acc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[h][i] = 0.f;
    const bool rowsum = RS && p.a_rowsum != nullptr && tn == 0 && wn == 0;   // wave-uniform; every k-split adds its share
    f32x16 accx;
#pragma unroll
    for (int i = 0; i < 16; ++i) accx[i] = 0.f;
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;
    bf16x8 fa[FM][BK / 16], fb[BK / 16], fb2[W2 ? BK / 16 : 1];
    constexpr int RK = FM * (A_KC ? 1 : 2) + (W2 ? 2 : 1) * (B_KC ? 1 : 2);
    static_assert(2 * RK <= 15, "the counted lgkmcnt of ws64_consume");
    // BM = 128, row sums: ONE more accumulator for both fragments.  The A fragment goes in as the B operand (same register layout)
    // against a 0 / 1 selector: rows 0-15 of the result carry the row sums of fragment 0 (column j = row j of A), rows 16-31 those
    // of fragment 1.
    bf16x8 sel[2];
    if constexpr (FM == 2 && RS) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            sel[0][i] = (__bf16)((lane & 16) ? 0.0f : 1.0f);
            sel[1][i] = (__bf16)((lane & 16) ? 1.0f : 0.0f);
        }
    }
    auto rd = [&](const unsigned char* TA, auto kk_c) {
        constexpr int kk = decltype(kk_c)::value;
        fa[0][kk] = frag_asm<BM, A_KC>(TA, wm * (BM / 2), kk, lane);
        if constexpr (FM == 2) fa[1][kk] = frag_asm<BM, A_KC>(TA, wm * (BM / 2) + 32, kk, lane);
        fb[kk] = frag_asm<BN, B_KC>(TA + A_T, wn * 32, kk, lane);
        if constexpr (W2) fb2[kk] = frag_asm<BN, B_KC>(TA + A_T + B_T, wn * 32, kk, lane);
    };
    auto mm = [&](auto kk_c) {
        constexpr int kk = decltype(kk_c)::value;
        if constexpr (FM == 2) {
            frag_tie(fa[0][kk]); frag_tie(fa[1][kk]); frag_tie(fb[kk]);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][kk], fb[kk], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][kk], fb[kk], acc[1], 0, 0, 0);
            if constexpr (RS) {
                if (rowsum) {
                    accx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sel[0], fa[0][kk], accx, 0, 0, 0);
                    accx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sel[1], fa[1][kk], accx, 0, 0, 0);
                }
            }
            return;
        }
        frag_tie(fa[0][kk]); frag_tie(fb[kk]);
        if constexpr (W2) {                                              // the small term first
            frag_tie(fb2[kk]);
            acc[kk & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][kk], fb2[kk], acc[kk & 1], 0, 0, 0);
        }
        acc[kk & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][kk], fb[kk], acc[kk & 1], 0, 0, 0);
        if constexpr (RS) {
            if (rowsum) accx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][kk], ones, accx, 0, 0, 0);
        }
    };
    // the bias of this wave's four-column groups, fetched now (after the loop it would cost an exposed memory latency)
    const int nq = n0 + wn * 32 + 4 * (lane % 8);
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (p.bias && nq < p.N) bias4 = *reinterpret_cast<const f32x4*>(p.bias + nq);
    stamp(0);
    wg_barrier();                                                        // B_0
    stamp(1);
    ws64_consume<2 * RK, S, STG>(smem, nk, rd, mm);
    if constexpr (FM == 2) {
        // (lane l of the lower half wave: result rows 0 and 16 — registers 0 and 8 — of column l = the sums of rows l of either fragment)
        if (RS && rowsum && hi == 0) {
            const int m = m0 + wm * 64 + l31;
            if (m < p.M) atomicAdd(p.a_rowsum + m, accx[0]);
            if (m + 32 < p.M) atomicAdd(p.a_rowsum + m + 32, accx[8]);
        }
    }
    if (FM == 1 && RS && rowsum && l31 == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm * 32 + crow(r, hi);
            if (m < p.M) atomicAdd(p.a_rowsum + m, accx[r]);
        }
    }
    // The tail (gemm_wsx3_body has a copy without the stamps).  As one shared function it changed the code of every kernel built on
    // either body (pairs of ds_write_b32 merged in the parked quadrant, other compare forms all over the epilogue, other register
    // counts on seven of the ten kernels): written out in both.
    stamp(2);                                                            // k-loop done
    f32x16 accs[1][FM];
    if constexpr (FM == 2) {
        accs[0][0] = acc[0]; accs[0][1] = acc[1];
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) accs[0][0][i] = acc[0][i] + acc[1][i];
    }
    // the epilogue's LDS (4 KB per wave, the split-K flag, the norm shares) ALIASES the stages: every consumer is past its last
    // fragment read at this barrier, every DMA has landed, and the producers are gone — so the whole LDS budget is prefetch depth
    __syncthreads();
    float* Tw = reinterpret_cast<float*>(smem) + wave * (1024 * FM);
    if (p.splits > 1) {
        // (the producers have left: these barriers count the four consumer waves only)
        const int tile = p.tile0 + tm * p.tiles_n + tn;
        float* part = p.ws + VITAE_GLDS_TICKETS + (long)tile * p.splits * (BM * BN);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(part, 0, p.splits * (BM * BN * 4), 0x00020000);
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const int toff = (int)threadIdx.x * 16;
#pragma unroll
        for (int g = 0; g < 4 * FM; ++g) {
            const f32x4 v = {accs[0][g >> 2][4 * (g & 3)], accs[0][g >> 2][4 * (g & 3) + 1], accs[0][g >> 2][4 * (g & 3) + 2], accs[0][g >> 2][4 * (g & 3) + 3]};
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (zid * (4 * FM) + g) * (256 * 16) + toff, 0, 16);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int* flag = reinterpret_cast<int*>(smem + 4 * 4096 * FM);
        if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add(reinterpret_cast<int*>(p.ws) + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        stamp(3);                                                        // partials parked, ticket taken
        if (*flag != p.splits - 1) return;
#pragma unroll
        for (int f = 0; f < FM; ++f)
#pragma unroll
            for (int i = 0; i < 16; ++i) accs[0][f][i] = 0.f;
        constexpr int SU = 4 / FM;                                       // splits in flight together: 16 loads of 16 bytes per lane
#pragma unroll 1
        for (int sp0 = 0; sp0 < p.splits; sp0 += SU) {
            f32x4 v[SU][4 * FM];
#pragma unroll
            for (int u = 0; u < SU; ++u) {
                const int sp = min(sp0 + u, p.splits - 1);               // (clamped: a repeated load, never added)
#pragma unroll
                for (int g = 0; g < 4 * FM; ++g)
                    v[u][g] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (sp * (4 * FM) + g) * (256 * 16) + toff, 0, 16));
            }
#pragma unroll
            for (int u = 0; u < SU; ++u)
                if (sp0 + u < p.splits) {
#pragma unroll
                    for (int g = 0; g < 4 * FM; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) accs[0][g >> 2][4 * (g & 3) + e] += v[u][g][e];
                }
        }
        if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<int*>(p.ws) + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    stamp(4);                                                            // epilogue starts
    bt_park_quadrant<FM, 1, 1>(accs, lane, Tw);
    __builtin_amdgcn_wave_barrier();
    float sqs = 0.f;
    { f32x4 cz = {0.f, 0.f, 0.f, 0.f}; bt_wave_epilogue<FM, 1, KINDS>(p, bt_epilogue_kind(p), m0 + wm * (BM / 2), n0 + wn * 32, Tw, lane, sqs, bias4, cz, false); }
    stamp(5);                                                            // stores issued
    if (p.sqacc) {                                                       // one atomic per workgroup (see bt_tail)
        sqs = wave_sum(sqs);
        float* red = reinterpret_cast<float*>(smem + 4 * 4096 * FM + 64);
        if (lane == 0) red[wave] = sqs;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(sq_slot(p), (double)((red[0] + red[1]) + (red[2] + red[3])));
    }
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(6); }      // stores drained
}

// the epilogue set of an operand form: forward (both k-contiguous), input gradient (A k-contiguous), weight gradient (neither)
template <bool A_KC, bool B_KC> constexpr int ws64_kinds() { return A_KC && B_KC ? BT_KINDS_FWD : A_KC ? BT_KINDS_DGRAD : BT_KINDS_WGRAD; }

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(64 * (4 + VITAE_WS64_PRODUCERS), 2) void gemm_ws64_kernel(WS_HOT_PARAMS, const GArgs p) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[WS64_SMEM];      // the ONLY LDS object
    const WsHot h = WS_HOT_FROM_PARAMS;
    gemm_ws64_body<A_KC, B_KC, VITAE_WS64_STAGES, false, false, 64, ws64_kinds<A_KC, B_KC>()>(p, h, blockIdx.x, blockIdx.z, smem);
}

// the 128 x 64 tile (id 7): [A 16 KB | B 8 KB] per stage, three stages = 72 KB, two workgroups per CU
constexpr int WS128X64_STAGES = 3, WS128X64_SMEM = WS128X64_STAGES * 24576;
template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(64 * (4 + VITAE_WS64_PRODUCERS), 2) void gemm_ws64_m128_kernel(WS_HOT_PARAMS, const GArgs p) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[WS128X64_SMEM];  // the ONLY LDS object
    const WsHot h{A, B, B2, lda, ldb, M, N, K, (M + 127) >> 7, (N + 63) >> 6, xcd_m, kps};
    gemm_ws64_body<A_KC, B_KC, WS128X64_STAGES, false, false, 128, ws64_kinds<A_KC, B_KC>()>(p, h, blockIdx.x, blockIdx.z, smem);
}

// id: 5 (64 x 64) or 7 (128 x 64); p.tiles_m / p.tiles_n are that tile's counts (bt_launch)
void ws64_launch(const GArgs& p, int a_kc, int b_kc, int id, hipStream_t st) {
    const dim3 grid(8 * cdiv((long)p.tiles_m * p.tiles_n, 8), 1, p.splits), block(64 * (4 + VITAE_WS64_PRODUCERS));
    if (id == 7) {
        if (a_kc && b_kc) hipLaunchKernelGGL((gemm_ws64_m128_kernel<true, true>), grid, block, 0, st, WS_HOT_ARGS(p), p);
        else if (a_kc && !b_kc) hipLaunchKernelGGL((gemm_ws64_m128_kernel<true, false>), grid, block, 0, st, WS_HOT_ARGS(p), p);
        else hipLaunchKernelGGL((gemm_ws64_m128_kernel<false, false>), grid, block, 0, st, WS_HOT_ARGS(p), p);
        return;
    }
    if (a_kc && b_kc) hipLaunchKernelGGL((gemm_ws64_kernel<true, true>), grid, block, 0, st, WS_HOT_ARGS(p), p);
    else if (a_kc && !b_kc) hipLaunchKernelGGL((gemm_ws64_kernel<true, false>), grid, block, 0, st, WS_HOT_ARGS(p), p);
    else hipLaunchKernelGGL((gemm_ws64_kernel<false, false>), grid, block, 0, st, WS_HOT_ARGS(p), p);
}

constexpr int WS64W2_STAGES = 3;           // [A | B hi | B lo] = 24 KB per stage: three stages = 72 KB, two workgroups per CU
__global__ __launch_bounds__(64 * (4 + VITAE_WS64_PRODUCERS), 2) void gemm_ws64_w2_kernel(WS_HOT_PARAMS, const GArgs p) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[WS64W2_STAGES * 24576];      // the ONLY LDS object
    gemm_ws64_body<true, true, WS64W2_STAGES, false, true, 64, BT_KINDS_FWD>(p, WS_HOT_FROM_PARAMS, blockIdx.x, blockIdx.z, smem);
}

// p: a complete forward-form descriptor (both operands k-contiguous, vec_epi set, p.B2 = the lo plane, p.splits k-ranges)
int ws64_w2_launch(GArgs p, hipStream_t st) {
    if (!p.vec_epi || !p.B2 || p.a_rowsum || (p.K % BK) || p.splits < 1) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (!bt_k_ranges(p.K, 2, p.splits, p.k_per_split)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    p.tiles_m = cdiv(p.M, 64); p.tiles_n = cdiv(p.N, 64); p.tile0 = 0;
    if (p.splits > 1 && (!p.ws || (long)p.tiles_m * p.tiles_n > VITAE_GLDS_TICKETS || p.epi == VITAE_EPI_GELU)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const dim3 grid(8 * cdiv((long)p.tiles_m * p.tiles_n, 8), 1, p.splits), block(64 * (4 + VITAE_WS64_PRODUCERS));
    hipLaunchKernelGGL(gemm_ws64_w2_kernel, grid, block, 0, st, WS_HOT_ARGS(p), p);
    return vitae_launch_status();
}

// Backward of one Linear as ONE launch of such workgroups: the first nb1 * p1.splits blocks compute the input gradient
// dx = epi(dy W) (A = dy k-contiguous, B = W row-contiguous; its long reduction cut into p1.splits), the rest the weight gradient
// dW (+)= dy^T x (both row-contiguous; RS: + colsum(dy)).
// The leading scalars are what either half needs before its first DMA (WsHot), in 14 dwords so that all of them are preloaded: the
// halves of one Linear's backward SHARE dy (A of both), its leading dimension, the leading dimension of W / x, the width K of the layer
// (N of both), and the weight gradient's rows are the input gradient's reduction length (ws64_pair_launch checks exactly that).
//   packed = nb1 | p1.splits << 20 | p1.xcd_m << 24 | p2.xcd_m << 25 | (dbg set) << 26 | (128-row input gradient) << 27 | (128-row weight gradient) << 28
// ONE image for every pair launch of a step: the rows of either half's tile (64: tile 5, 128: tile 7) travel in `packed`, and
// wave-uniform branches (a kernel argument and blockIdx: scalar) select among FOUR bodies, each instantiated once — 64-row and
// 128-row input gradient, 64-row and 128-row weight gradient, each as its producers' and its consumers' part — with the epilogue
// sets of their forms (BT_KINDS_DGRAD / _WGRAD).
// The row sums are a run-time property of both weight-gradient bodies (p2.a_rowsum; the predicate was wave-uniform and run-time
// already: the MFMAs against ones sit behind it).  As <RS, BM1, BM2> instantiations there were eight kernels of 265-512 KB whose
// sixteen inlined bodies each carried all 22 epilogue instantiations.
// LDS: the 72 KB of the 128-row geometry, static; the 64-row bodies keep their four 16 KB stages inside it.  Two workgroups per CU.
// p1 / p2 go to the bodies directly in the if / else chain (a select over two by-value descriptors: LABNOTES.md, round 6).
__global__ __launch_bounds__(64 * (4 + VITAE_WS64_PRODUCERS), 2) void gemm_ws64_pair_kernel(const __bf16* A, const __bf16* B1, const __bf16* B2, int lda, int ldb,
                                                                                           int M1, int N1, int K1, int K2, int kps1, int packed,
                                                                                           const GArgs p1, const GArgs p2) {
    static_assert(WS128X64_SMEM >= WS64_SMEM && 2 * WS128X64_SMEM <= 160 * 1024, "either body's stages; two workgroups per CU");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[WS128X64_SMEM];
    const int nb1 = packed & 0xfffff, splits1 = (packed >> 20) & 15, dbg2 = (packed >> 25) & 2;
    // The producer / consumer split comes FIRST, the half and its row count after it, so that no use of p1 / p2 is on the producers'
    // path: both row counts of a half read the same descriptor, and hipcc places those scalar loads (and their s_waitcnt, twice)
    // in front of the branch that the uses have in common.  With the row-count branch outermost that was in front of the tile
    // decode and the first DMA of every workgroup: every pair launch of the step 0.4-0.6 us longer (profiles/pair_image_*).
#define VITAE_WS64_PAIR_HALVES(ROLE)                                                                                                              \
    if ((int)blockIdx.x < nb1 * splits1) {                                                                                                        \
        if ((packed >> 27) & 1) {                                                                                                                 \
            const WsHot h{A, B1, nullptr, lda, ldb, M1, N1, K1, (M1 + 127) >> 7, (N1 + 63) >> 6, ((packed >> 24) & 1) | dbg2, kps1};             \
            gemm_ws64_body<true, false, WS128X64_STAGES, false, false, 128, BT_KINDS_DGRAD, ROLE>(p1, h, blockIdx.x % nb1, blockIdx.x / nb1, smem); \
        } else {                                                                                                                                  \
            const WsHot h{A, B1, nullptr, lda, ldb, M1, N1, K1, (M1 + 63) >> 6, (N1 + 63) >> 6, ((packed >> 24) & 1) | dbg2, kps1};              \
            gemm_ws64_body<true, false, VITAE_WS64_STAGES, false, false, 64, BT_KINDS_DGRAD, ROLE>(p1, h, blockIdx.x % nb1, blockIdx.x / nb1, smem); \
        }                                                                                                                                         \
    } else {                                                                                                                                      \
        if ((packed >> 28) & 1) {                                                                                                                 \
            const WsHot h{A, B2, nullptr, lda, ldb, K1, N1, K2, (K1 + 127) >> 7, (N1 + 63) >> 6, ((packed >> 25) & 1) | dbg2, K2};               \
            gemm_ws64_body<false, false, WS128X64_STAGES, true, false, 128, BT_KINDS_WGRAD, ROLE>(p2, h, blockIdx.x - nb1 * splits1, 0, smem);    \
        } else {                                                                                                                                  \
            const WsHot h{A, B2, nullptr, lda, ldb, K1, N1, K2, (K1 + 63) >> 6, (N1 + 63) >> 6, ((packed >> 25) & 1) | dbg2, K2};                \
            gemm_ws64_body<false, false, VITAE_WS64_STAGES, true, false, 64, BT_KINDS_WGRAD, ROLE>(p2, h, blockIdx.x - nb1 * splits1, 0, smem);   \
        }                                                                                                                                         \
    }
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= 4) {
        VITAE_WS64_PAIR_HALVES(1)
    } else {
        VITAE_WS64_PAIR_HALVES(2)
    }
#undef VITAE_WS64_PAIR_HALVES
}

// p1 / p2: complete descriptors of the two halves (vec_epi set, K % 64 == 0); p1.splits k-ranges of >= 2 k-tiles each;
// bm1 / bm2: the rows of either half's tile, 64 (tile 5) or 128 (tile 7)
int ws64_pair_launch(GArgs p1, GArgs p2, hipStream_t st, int bm1, int bm2) {
    if ((bm1 != 64 && bm1 != 128) || (bm2 != 64 && bm2 != 128)) return VITAE_ERR_INVALID_ARG;
    if (!p1.vec_epi || !p2.vec_epi || (p1.K % BK) || (p2.K % BK) || p2.K < 2 * BK || p1.a_rowsum) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (p1.splits < 1) p1.splits = 1;
    if (!bt_k_ranges(p1.K, 2, p1.splits, p1.k_per_split)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    p1.tiles_m = cdiv(p1.M, bm1); p1.tiles_n = cdiv(p1.N, 64); p1.tile0 = 0;
    p2.tiles_m = cdiv(p2.M, bm2); p2.tiles_n = cdiv(p2.N, 64); p2.tile0 = 0;
    p2.k_per_split = p2.K; p2.splits = 1;
    if (p1.splits > 1 && (!p1.ws || (long)p1.tiles_m * p1.tiles_n > VITAE_GLDS_TICKETS)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const int nb1 = 8 * cdiv((long)p1.tiles_m * p1.tiles_n, 8), nb2 = 8 * cdiv((long)p2.tiles_m * p2.tiles_n, 8);
    const dim3 grid(nb1 * p1.splits + nb2), block(64 * (4 + VITAE_WS64_PRODUCERS));
    // what the kernel's leading scalars assume (the two halves of ONE Linear's backward: gemm_ws64_pair_kernel)
    if (p1.A != p2.A || p1.lda != p2.lda || p1.ldb != p2.ldb || p2.M != p1.K || p2.N != p1.N || nb1 >= (1 << 20) || p1.splits > 15 ||
        p1.lda >= (1L << 31) || p1.ldb >= (1L << 31)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    const int packed = nb1 | p1.splits << 20 | (p1.xcd_m & 1) << 24 | (p2.xcd_m & 1) << 25 | ((p1.dbg || p2.dbg) ? 1 << 26 : 0) |
                       (bm1 == 128 ? 1 << 27 : 0) | (bm2 == 128 ? 1 << 28 : 0);
    hipLaunchKernelGGL(gemm_ws64_pair_kernel, grid, block, 0, st, p1.A, p1.B, p2.B, (int)p1.lda, (int)p1.ldb, p1.M, p1.N, p1.K, p2.K, p1.k_per_split,
                       packed, p1, p2);
    return vitae_launch_status();
}

}  // namespace vglds
