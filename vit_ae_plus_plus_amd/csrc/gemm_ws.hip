// Wave-specialised 128 x 128 and 128 x 256 tiles (tile ids 4 and 6) of the big-tile family, and their grouped weight-gradient
// kernels.  The dispatchers (bt_launch, bt_wgrad_group_launch) are in gemm_bt.hip; what the families share is in gemm_bt.hpp.
#include "gemm_bt.hpp"

namespace vglds {

// ---- wave-specialised 128 x 128 tile (tile id 4, round 4) --------------------------------------------------------------------
// Why: on the ping-pong 128 x 128 tile (gemm_bt.hip) every wave issues its own LDS-DMA pieces between its MFMAs.  A piece occupies the issuing wave
// for 60-180 clocks (the CU's texture addresser takes ~45 B/clk, and the wave sits at the instruction until its 1 KB is accepted):
// eight pieces per wave and k-tile are 500-1400 clocks during which that wave issues no MFMA — a lone workgroup runs ~1465 clocks
// per 64-deep k-tile for 512 clocks of MFMA, and two workgroups per CU are no faster (LABNOTES round-4 notes).  Here the roles are
// split: waves 0-3 (one per SIMD) only read fragments and issue MFMAs, waves 4-7 (their SIMD partners) only issue DMA.  A blocked
// DMA instruction stalls nobody but its own wave; the matrix pipe of the SIMD keeps running on the consumer wave.
//   * S stages of one whole k-tile (A 128 x 64 | B 128 x 64 = 32 KB); producers run S - 1 tiles ahead;
//   * ONE workgroup barrier per k-tile.  B_t (t = 0 .. nk - 1) promises: tile t has landed (every producer waited for its own
//     pieces of it with a counted vmcnt before arriving) and every fragment read of tile t - 1 has retired (every consumer waited
//     lgkmcnt(0) before arriving), so the producers restage tile t - 1's slot with tile t + S - 1 right after it;
//   * a consumer crosses B_{t+1} in the MIDDLE of k-tile t (after the MFMAs of k-slices 0-1, with the fragments of slices 2-3
//     already in registers) and reads slices 0-1 of tile t + 1 under the MFMAs of slices 2-3: no fragment-read latency is exposed
//     at a tile boundary;
//   * producers leave after the last barrier; the consumers run the family's tail (in-launch split-K fix-up, wave-private epilogue).
#ifndef VITAE_WS_STAGES
#define VITAE_WS_STAGES 3         // (3 / 4 / 5 stages measured alike — the deeper ones with the tail's LDS aliasing the stages, LABNOTES round 5: the
                                  // loop sits on the CU's L2 -> LDS feed, 32 KB per ~870 clocks = 37 B/clk, not on its latency)
#endif
#ifndef VITAE_WS_TAIL8
#define VITAE_WS_TAIL8 1          // unsplit launches: the producer waves take half of the epilogue (quadrants A-hi x B-lo / B-hi of their SIMD partner)
#endif
#ifndef VITAE_WS_INTERLEAVE
#define VITAE_WS_INTERLEAVE 1     // fragment reads one per MFMA gap (round 5) instead of bursts of eight between the MFMA blocks
#endif
#ifndef VITAE_WS_FINE_STAMPS
#define VITAE_WS_FINE_STAMPS 0    // 1: s_memtime stamps inside ONE k-tile of the consumer (variant library for tools/ws_phase_probe.py fine)
#endif
constexpr int WS_SMEM = VITAE_WS_STAGES * 32768 + (VITAE_WS_TAIL8 ? 12 * 4096 + 64 : 0);      // the stages, and behind them the tail's LDS
template <bool A_KC, bool B_KC, int S>
__device__ __forceinline__ void gemm_ws_body(const GArgs& p, const int bid, const int zid, unsigned char* smem) {
    constexpr int BM = 128, BN = 128, NWC = 4, NWP = 4;
    constexpr int A_T = BM * BK * 2, B_T = BN * BK * 2, STG = A_T + B_T;
    constexpr int PA = pieces<BM, A_KC, NWP>(), PB = pieces<BN, B_KC, NWP>(), PT = PA + PB;
    constexpr int TAILOFF = S * STG;                                 // byte offset of the tail's LDS (parked quadrants, wave-private staging)
    static_assert(S >= 3 && S <= 5 && S * STG + (VITAE_WS_TAIL8 ? 12 * 4096 + 64 : 0) <= 160 * 1024 && (S - 2) * PT <= 63, "stages fit LDS, three tiles of pieces fit the vmcnt field");
    // the XCD-balanced tile map (gemm_bt.hpp)
    const int T = p.tiles_m * p.tiles_n;
    const int xq = T >> 3, xr = T & 7, xcd = bid & 7;
    const int lin = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
    if ((bid >> 3) >= xq + (xcd < xr ? 1 : 0)) return;
    const int tn = p.xcd_m ? lin % p.tiles_n : lin / p.tiles_m;
    const int tm = p.xcd_m ? lin / p.tiles_n : lin % p.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = zid * p.k_per_split;
    const int nk = (min(p.K, kbeg + p.k_per_split) - kbeg) / BK;         // >= 2 (launcher)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto stamp = [&](int i) {
        if (p.dbg && lane == 0 && (wave & 3) == 0) p.dbg[(((long)zid * (8 * ((T + 7) >> 3)) + bid) * 2 + (wave >> 2)) * 32 + i] = __builtin_amdgcn_s_memtime();
    };
    stamp(0);

    if (wave >= NWC) {
        // ---------------- producers: DMA only ----------------
        const int pw = wave - NWC;
        auto issue_tile = [&](int t, int stage) {
            unsigned char* dst = smem + stage * STG;
            const int k0 = kbeg + t * BK;
#pragma unroll
            for (int j = 0; j < PA; ++j) dma_piece<BM, A_KC, NWP>(p.A, p.lda, p.M, m0, a_wrap(p, k0), dst, pw, lane, j);
#pragma unroll
            for (int j = 0; j < PB; ++j) dma_piece<BN, B_KC, NWP>(p.B, p.ldb, p.N, n0, k0, dst + A_T, pw, lane, j);
        };
        const int npre = min(S - 1, nk);
        const bool active = pw < NWP;
        for (int t = 0; t < npre; ++t) if (active) issue_tile(t, t);
        wait_tiles<S, PT>(npre - 1);
        wg_barrier();                                                    // B_0
        int stage = npre % S;                                            // slot of tile t + S - 1 (= tile t - 1's)
#pragma unroll 1
        for (int t = 0; t + 1 < nk; ++t) {
            const bool pr = p.dbg && t >= 3 && t < 9;                    // tools/ws_phase_probe.py: who arrives last at B_4 .. B_9
            if (t + S - 1 < nk) {
                if (active) issue_tile(t + S - 1, stage);
                stage = stage + 1 == S ? 0 : stage + 1;
            }
            if (pr) stamp(2 + 3 * (t - 3));                               // pieces issued
            wait_tiles<S, PT>(min(t + S - 1, nk - 1) - (t + 1));         // B_{t+1}: tile t + 1 has landed
            if (pr) stamp(3 + 3 * (t - 3));                               // arrival
            wg_barrier();
            if (pr) stamp(4 + 3 * (t - 3));                               // departure
        }
        if (!VITAE_WS_TAIL8 || p.splits > 1) return;                     // (split launches: the consumers' fix-up has barriers of its own)
        // the epilogue of the partner's two A-hi quadrants, parked by it in this wave's two LDS regions behind the stages
        const int wmp = pw >> 1, wnp = pw & 1;
        f32x4 bq[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int n = n0 + b * 64 + wnp * 32 + 4 * (lane % 8);
            bq[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p.bias && n < p.N) bq[b] = *reinterpret_cast<const f32x4*>(p.bias + n);
        }
        const int kind = bt_epilogue_kind(p);
        const float* Pq = reinterpret_cast<const float*>(smem + TAILOFF) + pw * 2048;
        float sqs = 0.f;
        wg_barrier();                                                    // T: the partner's quadrants are in LDS
#pragma unroll 1
        for (int b = 0; b < 2; ++b) { f32x4 cz = {0.f, 0.f, 0.f, 0.f}; bt_wave_epilogue<1, 1>(p, kind, m0 + 64 + wmp * 32, n0 + b * 64 + wnp * 32, Pq + b * 1024, lane, sqs, b ? bq[1] : bq[0], cz, false); }
        if (p.sqacc) {                                                   // one atomic per workgroup (see bt_tail)
            sqs = wave_sum(sqs);
            float* red = reinterpret_cast<float*>(smem + TAILOFF + 12 * 4096);
            if (lane == 0) red[wave] = sqs;
            wg_barrier();
        }
        return;
    }

    // ---------------- consumers: fragment reads + MFMA ----------------
    const int wm = wave >> 1, wn = wave & 1;
    f32x16 acc[2][2][1][1];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][0][0][i] = 0.f;
    bf16x8 fa[BK / 16][2], fb[BK / 16][2];
    constexpr int RK = (A_KC ? 2 : 4) + (B_KC ? 2 : 4);                 // LDS instructions of one k-slice's fragments
    constexpr int W2 = 2 * RK > 15 ? 15 : 2 * RK;
    auto rd = [&](const unsigned char* TA, auto kk_c) {
        constexpr int kk = decltype(kk_c)::value;
        const unsigned char* TB = TA + A_T;
#pragma unroll
        for (int h = 0; h < 2; ++h) fa[kk][h] = frag_asm<BM, A_KC>(TA, h * 64 + wm * 32, kk, lane);
#pragma unroll
        for (int h = 0; h < 2; ++h) fb[kk][h] = frag_asm<BN, B_KC>(TB, h * 64 + wn * 32, kk, lane);
    };
    auto mm = [&](auto kk_c) {
        constexpr int kk = decltype(kk_c)::value;
#pragma unroll
        for (int h = 0; h < 2; ++h) { frag_tie(fa[kk][h]); frag_tie(fb[kk][h]); }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b][0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kk][a], fb[kk][b], acc[a][b][0][0], 0, 0, 0);
    };
    wg_barrier();                                                        // B_0: tile 0 is in LDS
    rd(smem, K0{}); rd(smem, K1{});
    int stage = 0;
#if VITAE_WS_INTERLEAVE
    // Round 5 (tools/ws_phase_probe.py): the k-loop was bound by the CONSUMER — every barrier found the producers waiting 200-330
    // clocks, the interval was 1080 clocks for 512 of MFMA.  An in-order wave that issues eight fragment reads in a burst sits at
    // them for 100-300 clocks (four waves share the LDS port with the DMA's writes) while its matrix pipe drains.  Here the reads of
    // the two slices ahead are issued ONE FRAGMENT PER MFMA GAP: the four MFMAs of a slice carry the eight fragments of the next
    // pair of slices (each read issues in the 32-clock shadow of the MFMA in front of it).
    //   slice 0 MFMAs + reads of slices 2, 3 | slice 1 MFMAs | all reads of tile t retired, B_{t+1} | slice 2 MFMAs + reads of the
    //   next tile's slices 0, 1 | slice 3 MFMAs
    const FragOff<BM, A_KC> offa = frag_offsets<BM, A_KC>(wm * 32, lane);
    const FragOff<BN, B_KC> offb = frag_offsets<BN, B_KC>(wn * 32, lane);
    typedef __attribute__((address_space(3))) const unsigned char lds_u8;
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_u8*)smem;
    // Eight MFMAs (k-slices S0, S0 + 1) that carry the eight fragments of slices R0, R0 + 1 of the tile at LDS address `rb`:
    // gap:       0        1      2      3        4      5     6  7
    // fragments  a0 b0    a0'    b0'    a1 b1    a1'    b1'   -  -      (x' = the half 64 rows further; the last two gaps stay
    // empty so that the lgkmcnt(0) behind the block finds every read retired)
    auto half = [&](auto s0_c, const unsigned rb, auto r0_c, bool do_rd) {
        constexpr int S0 = decltype(s0_c)::value, R0 = decltype(r0_c)::value;
#pragma unroll
        for (int k = S0; k < S0 + 2; ++k)
#pragma unroll
            for (int h = 0; h < 2; ++h) { frag_tie(fa[k][h]); frag_tie(fb[k][h]); }
        __builtin_amdgcn_sched_barrier(0);
        unsigned aa = 0, ab = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = S0 + (j >> 2), a = (j >> 1) & 1, b = j & 1;
            acc[a][b][0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kk][a], fb[kk][b], acc[a][b][0][0], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (do_rd && j < 6) {
                if (j == 0) {
                    aa = frag_base<BM, A_KC, R0>(rb, offa, 0); ab = frag_base<BN, B_KC, R0>(rb + A_T, offb, 0);
                    fa[R0][0] = frag_rd<BM, A_KC, R0, 0>(aa); fb[R0][0] = frag_rd<BN, B_KC, R0, 0>(ab);
                }
                if (j == 1) { if (!A_KC) aa = frag_base<BM, A_KC, R0>(rb, offa, 1); fa[R0][1] = frag_rd<BM, A_KC, R0, A_KC ? 1 : 0>(aa); }
                if (j == 2) { if (!B_KC) ab = frag_base<BN, B_KC, R0>(rb + A_T, offb, 1); fb[R0][1] = frag_rd<BN, B_KC, R0, B_KC ? 1 : 0>(ab); }
                if (j == 3) {
                    aa = frag_base<BM, A_KC, R0 + 1>(rb, offa, 0); ab = frag_base<BN, B_KC, R0 + 1>(rb + A_T, offb, 0);
                    fa[R0 + 1][0] = frag_rd<BM, A_KC, R0 + 1, 0>(aa); fb[R0 + 1][0] = frag_rd<BN, B_KC, R0 + 1, 0>(ab);
                }
                if (j == 4) { if (!A_KC) aa = frag_base<BM, A_KC, R0 + 1>(rb, offa, 1); fa[R0 + 1][1] = frag_rd<BM, A_KC, R0 + 1, A_KC ? 1 : 0>(aa); }
                if (j == 5) { if (!B_KC) ab = frag_base<BN, B_KC, R0 + 1>(rb + A_T, offb, 1); fb[R0 + 1][1] = frag_rd<BN, B_KC, R0 + 1, B_KC ? 1 : 0>(ab); }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
#pragma unroll 1
    for (int t = 0; t < nk; ++t) {
        // entry: the fragments of slices 0, 1 of tile t were read under the MFMAs of the previous tile's slices 2, 3
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        half(K0{}, lds0 + stage * STG, K2{}, true);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // every read of tile t has retired (the last one two MFMAs ago)
        const bool more = t + 1 < nk;
        if (more) {
            wg_barrier();                                                   // B_{t+1}
            stage = stage + 1 == S ? 0 : stage + 1;
        }
        __builtin_amdgcn_s_setprio(1);
        half(K2{}, lds0 + stage * STG, K0{}, more);
        __builtin_amdgcn_s_setprio(0);
    }
#else
#pragma unroll 1
    for (int t = 0; t < nk; ++t) {
        const unsigned char* TA = smem + stage * STG;
#if VITAE_WS_FINE_STAMPS
        const bool fine = p.dbg && t == 12;                              // tools/ws_phase_probe.py fine: the pieces of ONE k-tile (perturbs the pipeline)
        if (fine) stamp(21);
#endif
        __builtin_amdgcn_sched_barrier(0);
        rd(TA, K2{}); rd(TA, K3{});
        __builtin_amdgcn_sched_barrier(0);
#if VITAE_WS_FINE_STAMPS
        if (fine) stamp(22);
#endif
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(W2) : "memory");     // slices 0-1 (read one barrier ago) are in registers
        __builtin_amdgcn_sched_barrier(0);
#if VITAE_WS_FINE_STAMPS
        if (fine) stamp(23);
#endif
        __builtin_amdgcn_s_setprio(1);
        mm(K0{}); mm(K1{});
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
#if VITAE_WS_FINE_STAMPS
        if (fine) stamp(24);
#endif
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // every read of tile t has retired: its slot may be restaged
        if (t + 1 < nk) {
            const bool pr = p.dbg && t >= 3 && t < 9;
            if (pr) stamp(2 + 3 * (t - 3));                               // arrival at B_{t+1}
#if VITAE_WS_FINE_STAMPS
            if (fine) stamp(25);
#endif
            wg_barrier();                                                   // B_{t+1}
            if (pr) stamp(3 + 3 * (t - 3));                               // departure
#if VITAE_WS_FINE_STAMPS
            if (fine) stamp(26);
#endif
            stage = stage + 1 == S ? 0 : stage + 1;
            const unsigned char* TN = smem + stage * STG;
            rd(TN, K0{}); rd(TN, K1{});
            __builtin_amdgcn_sched_barrier(0);
#if VITAE_WS_FINE_STAMPS
            if (fine) stamp(27);
#endif
        }
        __builtin_amdgcn_s_setprio(1);
        mm(K2{}); mm(K3{});
        __builtin_amdgcn_s_setprio(0);
#if VITAE_WS_FINE_STAMPS
        if (fine) stamp(28);
#endif
    }
#endif
    stamp(20);
    if (VITAE_WS_TAIL8 && p.splits == 1) {
        // unsplit launch: quadrants (A-hi, B-lo) and (A-hi, B-hi) go to the SIMD partner (a producer wave, idle by now) through
        // its two 4 KB regions behind the stages; this wave keeps (A-lo, B-lo) and (A-lo, B-hi).  Nothing here touches the stages,
        // which slower waves may still be reading.
        float* Pq = reinterpret_cast<float*>(smem + TAILOFF) + wave * 2048;
        float* Tw = reinterpret_cast<float*>(smem + TAILOFF) + 4 * 2048 + wave * 1024;
        f32x4 bq[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int n = n0 + b * 64 + wn * 32 + 4 * (lane % 8);
            bq[b] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (p.bias && n < p.N) bq[b] = *reinterpret_cast<const f32x4*>(p.bias + n);
        }
        const int kind = bt_epilogue_kind(p);
        bt_park_quadrant<1, 1, 1>(acc[1][0], lane, Pq);
        bt_park_quadrant<1, 1, 1>(acc[1][1], lane, Pq + 1024);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // the parked values are in LDS before the partner is released
        wg_barrier();                                                       // T
        float sqs = 0.f;
#pragma unroll 1
        for (int b = 0; b < 2; ++b) {
            if (b == 0) bt_park_quadrant<1, 1, 1>(acc[0][0], lane, Tw);
            else bt_park_quadrant<1, 1, 1>(acc[0][1], lane, Tw);
            __builtin_amdgcn_wave_barrier();
            { f32x4 cz = {0.f, 0.f, 0.f, 0.f}; bt_wave_epilogue<1, 1>(p, kind, m0 + wm * 32, n0 + b * 64 + wn * 32, Tw, lane, sqs, b ? bq[1] : bq[0], cz, false); }
            __builtin_amdgcn_wave_barrier();
        }
        if (p.sqacc) {
            sqs = wave_sum(sqs);
            float* red = reinterpret_cast<float*>(smem + TAILOFF + 12 * 4096);
            if (lane == 0) red[wave] = sqs;
            wg_barrier();
            if (threadIdx.x == 0) {
                float tot = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) tot += red[w];
                atomicAdd(sq_slot(p), (double)tot);
            }
        }
        return;
    }
    bt_tail<BM, BN, 2, 2, 1>(p, acc, smem, m0, n0, tm, tn, zid, wave, lane, stamp);
}

template <bool A_KC, bool B_KC>
__global__ __launch_bounds__(512, 2) void gemm_ws_kernel(const GArgs p) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[WS_SMEM];      // the ONLY LDS object
    gemm_ws_body<A_KC, B_KC, VITAE_WS_STAGES>(p, blockIdx.x, blockIdx.z, smem);
}

// ---- a 128 x 256 tile of the same structure for the WEIGHT-GRADIENT form (tile id 6; both operands row-contiguous) ---------------
// Why (round 5): the wave-specialised loop is bound by the CU's L2 -> LDS rate (37 B/clk), so what a k-tile costs is its BYTES:
// 32 KB for 128 x 128 (870 clocks), 48 KB for 128 x 256 (~1300) — 1.34x the outputs per byte.  A block's four weight gradients are
// 432 tiles of 128 x 128 on 256 one-workgroup-per-CU slots (1.69 rounds = 2); as 216 tiles of 128 x 256 they are ONE round.  The
// consumers keep the 2 x 2 arrangement of the family's tail (BtCfg<128, 256, 2, 2>: a wave owns rows a * 64 + wm * 32 and columns
// b * 128 + wn * 64 + f * 32, a, b, f in {0, 1}: eight 32 x 32 accumulators); eight MFMAs per k-slice carry the six fragments of a
// slice two ahead, one per MFMA gap.  Three stages of 48 KB; the tail (split fix-up, wave-private epilogue) aliases them.
template <int S>
__device__ __forceinline__ void gemm_wsw_body(const GArgs& p, const int bid, const int zid, unsigned char* smem) {
    constexpr int BM = 128, BN = 256, NWC = 4, NWP = 4;
    constexpr int A_T = BM * BK * 2, B_T = BN * BK * 2, STG = A_T + B_T;
    constexpr int PA = pieces<BM, false, NWP>(), PB = pieces<BN, false, NWP>(), PT = PA + PB;
    static_assert(S == 3 && S * STG <= 160 * 1024 && (S - 2) * PT <= 63, "three stages fit LDS, one tile of pieces fits the vmcnt field");
    // the XCD-balanced tile map (gemm_bt.hpp)
    const int T = p.tiles_m * p.tiles_n;
    const int xq = T >> 3, xr = T & 7, xcd = bid & 7;
    const int lin = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
    if ((bid >> 3) >= xq + (xcd < xr ? 1 : 0)) return;
    const int tn = p.xcd_m ? lin % p.tiles_n : lin / p.tiles_m;
    const int tm = p.xcd_m ? lin / p.tiles_n : lin % p.tiles_m;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = zid * p.k_per_split;
    const int nk = (min(p.K, kbeg + p.k_per_split) - kbeg) / BK;         // >= 2 (launcher)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    auto stamp = [&](int) {};

    if (wave >= NWC) {
        // ---------------- producers: DMA only (the protocol of gemm_ws_body) ----------------
        const int pw = wave - NWC;
        auto issue_tile = [&](int t, int stage) {
            unsigned char* dst = smem + stage * STG;
            const int k0 = kbeg + t * BK;
#pragma unroll
            for (int j = 0; j < PA; ++j) dma_piece<BM, false, NWP>(p.A, p.lda, p.M, m0, k0, dst, pw, lane, j);
#pragma unroll
            for (int j = 0; j < PB; ++j) dma_piece<BN, false, NWP>(p.B, p.ldb, p.N, n0, k0, dst + A_T, pw, lane, j);
        };
        const int npre = min(S - 1, nk);
        for (int t = 0; t < npre; ++t) issue_tile(t, t);
        wait_tiles<S, PT>(npre - 1);
        wg_barrier();                                                       // B_0
        int stage = npre % S;
#pragma unroll 1
        for (int t = 0; t + 1 < nk; ++t) {
            if (t + S - 1 < nk) {
                issue_tile(t + S - 1, stage);
                stage = stage + 1 == S ? 0 : stage + 1;
            }
            wait_tiles<S, PT>(min(t + S - 1, nk - 1) - (t + 1));         // B_{t+1}: tile t + 1 has landed
            wg_barrier();
        }
        return;                                                          // (a barrier only counts living waves: the tail belongs to the consumers)
    }

    // ---------------- consumers ----------------
    const int wm = wave >> 1, wn = wave & 1;
    f32x16 acc[2][2][1][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[a][b][0][f][i] = 0.f;
    bf16x8 fa[BK / 16][2], fb[BK / 16][4];
    // per-lane offsets inside a stage, computed once: A fragments at rows wm * 32 (+ 64), B fragments at columns wn * 64 + {0, 32, 128, 160}
    const FragOff<BM, false> offa = frag_offsets<BM, false>(wm * 32, lane);
    unsigned ob[4];
    {
        constexpr int LB = BN * 2;
        const int gg = lane >> 4, li = lane & 15;
        const int kl = 8 * (gg >> 1) + (li >> 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int col = wn * 64 + (i >> 1) * 128 + (i & 1) * 32 + 16 * (gg & 1) + 4 * (li & 3);
            ob[i] = A_T + kl * LB + (((col >> 3) ^ swz<false, BN / 8>(kl)) << 4) + (col & 7) * 2;
        }
    }
    typedef __attribute__((address_space(3))) const unsigned char lds_u8;
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_u8*)smem;
    // all six fragments of k-slice KK of the tile at LDS address rb
    auto rd_slice = [&](const unsigned rb, auto kk_c) {
        constexpr int KK = decltype(kk_c)::value;
        fa[KK][0] = frag_rd<BM, false, KK, 0>(rb + offa.o[0]);
        fa[KK][1] = frag_rd<BM, false, KK, 0>(rb + offa.o[1]);
#pragma unroll
        for (int i = 0; i < 4; ++i) fb[KK][i] = frag_rd<BN, false, KK, 0>(rb + ob[i]);
    };
    // Sixteen MFMAs (k-slices S0, S0 + 1) that carry the twelve fragments of slices R0, R0 + 1 of the tile at `rb`, one per gap
    // (the last four gaps stay empty: the lgkmcnt(0) behind the block finds every read retired)
    auto half = [&](auto s0_c, const unsigned rb, auto r0_c, bool do_rd) {
        constexpr int S0 = decltype(s0_c)::value, R0 = decltype(r0_c)::value;
#pragma unroll
        for (int k = S0; k < S0 + 2; ++k) {
            frag_tie(fa[k][0]); frag_tie(fa[k][1]);
#pragma unroll
            for (int i = 0; i < 4; ++i) frag_tie(fb[k][i]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int kk = S0 + (j >> 3), a = (j >> 2) & 1, bf = j & 3;
            acc[a][bf >> 1][0][bf & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kk][a], fb[kk][bf], acc[a][bf >> 1][0][bf & 1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (do_rd && j < 12) {
                if (j == 0) fa[R0][0] = frag_rd<BM, false, R0, 0>(rb + offa.o[0]);
                if (j == 1) fb[R0][0] = frag_rd<BN, false, R0, 0>(rb + ob[0]);
                if (j == 2) fa[R0][1] = frag_rd<BM, false, R0, 0>(rb + offa.o[1]);
                if (j == 3) fb[R0][1] = frag_rd<BN, false, R0, 0>(rb + ob[1]);
                if (j == 4) fb[R0][2] = frag_rd<BN, false, R0, 0>(rb + ob[2]);
                if (j == 5) fb[R0][3] = frag_rd<BN, false, R0, 0>(rb + ob[3]);
                if (j == 6) fa[R0 + 1][0] = frag_rd<BM, false, R0 + 1, 0>(rb + offa.o[0]);
                if (j == 7) fb[R0 + 1][0] = frag_rd<BN, false, R0 + 1, 0>(rb + ob[0]);
                if (j == 8) fa[R0 + 1][1] = frag_rd<BM, false, R0 + 1, 0>(rb + offa.o[1]);
                if (j == 9) fb[R0 + 1][1] = frag_rd<BN, false, R0 + 1, 0>(rb + ob[1]);
                if (j == 10) fb[R0 + 1][2] = frag_rd<BN, false, R0 + 1, 0>(rb + ob[2]);
                if (j == 11) fb[R0 + 1][3] = frag_rd<BN, false, R0 + 1, 0>(rb + ob[3]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    wg_barrier();                                                           // B_0: tile 0 is in LDS
    rd_slice(lds0, K0{}); rd_slice(lds0, K1{});
    int stage = 0;
#pragma unroll 1
    for (int t = 0; t < nk; ++t) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        half(K0{}, lds0 + stage * STG, K2{}, true);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // every read of tile t has retired
        const bool more = t + 1 < nk;
        if (more) {
            wg_barrier();                                                   // B_{t+1}
            stage = stage + 1 == S ? 0 : stage + 1;
        }
        __builtin_amdgcn_s_setprio(1);
        half(K2{}, lds0 + stage * STG, K0{}, more);
        __builtin_amdgcn_s_setprio(0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bt_tail<BM, BN, 2, 2, 1>(p, acc, smem, m0, n0, tm, tn, zid, wave, lane, stamp);
}

// A group of weight-gradient problems (BtGroup) on the wave-specialised 128 x 128 workgroup (one per CU): a k-tile of the
// weight-gradient form costs it ~900 clocks against ~1300 per tile for the two co-resident ping-pong workgroups of
// gemm_bt_wgrad_group_kernel (both operands come through the transposing reads, and there the waves that wait for them are the
// ones that multiply).
__global__ __launch_bounds__(512, 2) void gemm_ws_wgrad_group_kernel(const BtGroup g) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[WS_SMEM];
    const int b = blockIdx.x;
    const int i = bt_group_index(g, b);
    gemm_ws_body<false, false, VITAE_WS_STAGES>(g.p[i], b - g.start[i], blockIdx.z, smem);
}

// ... and on 128 x 256 tiles of it (gemm_wsw_body): 216 tiles instead of 432 for an encoder block — one round of the 256 slots
__global__ __launch_bounds__(512, 2) void gemm_wsw_wgrad_group_kernel(const BtGroup g) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[3 * 49152];
    const int b = blockIdx.x;
    const int i = bt_group_index(g, b);
    gemm_wsw_body<3>(g.p[i], b - g.start[i], blockIdx.z, smem);
}

void ws_launch(const GArgs& p, int a_kc, int b_kc, int id, hipStream_t st) {
    if (id == 6) {
        // (through the group kernel as a group of one: the stand-alone instantiation of the same body came out of hipcc with 136
        // spilled registers, the group one with 4)
        BtGroup g;
        const int total = 8 * cdiv(p.tiles_m * p.tiles_n, 8);
        for (int i = 0; i < 4; ++i) { g.p[i] = p; g.start[i] = i ? total : 0; }
        g.start[4] = total;
        hipLaunchKernelGGL(gemm_wsw_wgrad_group_kernel, dim3(total, 1, p.splits), dim3(512), 0, st, g);
        return;
    }
    const dim3 grid(8 * cdiv((long)p.tiles_m * p.tiles_n, 8), 1, p.splits), block(512);
    if (a_kc && b_kc) hipLaunchKernelGGL((gemm_ws_kernel<true, true>), grid, block, 0, st, p);
    else if (a_kc && !b_kc) hipLaunchKernelGGL((gemm_ws_kernel<true, false>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((gemm_ws_kernel<false, false>), grid, block, 0, st, p);
}

void ws_wgrad_group_launch(const BtGroup& g, int total, int splits, int kind, hipStream_t st) {
    if (kind == 2) hipLaunchKernelGGL(gemm_wsw_wgrad_group_kernel, dim3(total, 1, splits), dim3(512), 0, st, g);
    else hipLaunchKernelGGL(gemm_ws_wgrad_group_kernel, dim3(total, 1, splits), dim3(512), 0, st, g);
}

}  // namespace vglds
