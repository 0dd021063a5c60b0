// Big-tile bf16 GEMM (128x128 ... 256x256 per workgroup) for the launches that have enough rows to fill the chip with such
// tiles: decoder_pred at every batch size, every Linear of the step from batch 8-16 up, the patch-8 model.
//   C[M,N] (+)= epi( sum_k A(m,k) * B(n,k) + bias[n] ) (+ residual)      (operand storage flags as in gemm_glds.hip)
//
// Why a second kernel family: a 64x64 tile moves 16 KB of operands L2 -> LDS per 64-deep k-step for 64x64x64 MACs, and a CU
// takes at most ~46-56 B/clk from L2 (profiles/round2_probe_dma_pattern.txt; the L2's 34.5 TB/s over 256 CUs): ~330 clocks
// of feed for 128 clocks of MFMA.  A 256x256 tile moves 64 KB for 16x the MACs (1300 clocks of feed under 2048 of MFMA).
//
// Schedule (the 8-phase structure of cdna_hip_programming.md §5 "256^2 template", re-derived for this operand layout):
//   * a k-tile (64 deep) of each operand is staged as TWO half-tiles (A-lo | A-hi, B-lo | B-hi: HM = BM/2, HN = BN/2 rows
//     each), and every wave owns rows of BOTH halves: its (BM/WM) x (BN/WN) outputs are four quadrants (A-half x B-half);
//   * a k-tile is four phases, one quadrant each: P1 reads A-lo + B-lo fragments, P2 B-hi, P3 A-hi, P4 nothing (B-lo kept):
//     (A0,B0) (A0,B1) (A1,B1) (A1,B0) — at most A-half + 2 B-half fragments live (64 VGPRs at 256x256);
//   * two LDS buffers only, yet ~5 phases of prefetch distance: a half-tile's slot is free two phases after its last
//     fragment read, so the DMA of k-tile t + 2 starts in P3 of k-tile t, half-tile by half-tile (A-lo, B-lo, then B-hi and
//     A-hi in P1 / P2 of k-tile t + 1), always 4 half-tiles (64 KB at 256x256) in flight, retired by COUNTED vmcnt waits;
//   * 8-wave workgroups run as two groups of four waves (one per SIMD each) staggered by one barrier: while one group
//     issues its 8 MFMAs of a quadrant, the other issues DMA + fragment reads, so a SIMD's matrix pipe always has one of
//     its two waves in an MFMA segment.  4-wave workgroups (128x128) are not staggered: two of them share a CU.
// Hazards, by barrier count (slot = interval between two workgroup barriers; a phase = load slot + MFMA slot; group 1 runs one
// slot behind group 0): a half-tile needed by the reads of phase g + 1 is waited for (each wave: its own DMA pieces) in the
// load slot of phase g, i.e. >= 1 barrier before anyone reads it; a half-tile is re-staged >= 2 phases after its last read,
// i.e. >= 2 barriers after the lgkmcnt(0) that retired the slower group's reads.
#include "gemm_bt.hpp"

namespace vglds {

template <int BM, int BN, int WM, int WN, bool A_KC, bool B_KC>
__device__ __forceinline__ void gemm_bt_body(const GArgs& p, const int bid, const int zid, unsigned char* smem) {
    using Cf = BtCfg<BM, BN, WM, WN>;
    constexpr int NW = Cf::NW, HM = Cf::HM, HN = Cf::HN, FM = Cf::FM, FN = Cf::FN, NF = FM * FN;
    constexpr int A_HALF = Cf::A_HALF, B_HALF = Cf::B_HALF, BUF = Cf::BUF;
    constexpr bool STAGGER = NW == 8;
    constexpr int PA = pieces<HM, A_KC, NW>(), PB = pieces<HN, B_KC, NW>();
    constexpr int NACC = NF == 1 ? 2 : 1;          // one fragment per quadrant: even / odd k-slices on separate accumulators
    constexpr bool ASM_READS = !A_KC || !B_KC;     // transposing reads are inline asm: ordered by hand
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
    const int wm = wave / WN, wn = wave % WN;
    const bool late = STAGGER && wave >= 4;         // group 1: one barrier behind
    // tools/bt_phase_probe.py: shader-clock stamps of wave 0 / wave 4 (one per stagger group), 32 per (workgroup, group)
    auto stamp = [&](int i) {
        if (p.dbg && lane == 0 && (wave & 3) == 0) p.dbg[(((long)zid * (8 * ((T + 7) >> 3)) + bid) * 2 + (wave >> 2)) * 32 + i] = __builtin_amdgcn_s_memtime();
    };
    stamp(0);

    f32x16 acc[2][2][NACC][NF];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int h = 0; h < NACC; ++h)
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[a][b][h][f][i] = 0.f;

    // half-tile positions in issue order: 0 A-lo, 1 B-lo, 2 B-hi, 3 A-hi; LDS image of a buffer: [A-lo][A-hi][B-lo][B-hi]
    // one DMA instruction (piece j of this wave) of a half-tile
    auto issue_piece = [&](auto pos_c, int tile, int buf, int j) {
        constexpr int POS = decltype(pos_c)::value;
        constexpr int OFF = POS == 0 ? 0 : POS == 3 ? A_HALF : POS == 1 ? 2 * A_HALF : 2 * A_HALF + B_HALF;
        unsigned char* dst = smem + buf * BUF + OFF;
        const int k0 = kbeg + tile * BK;
        if constexpr (POS == 0 || POS == 3) dma_piece<HM, A_KC, NW>(p.A, p.lda, p.M, m0 + (POS == 3 ? HM : 0), a_wrap(p, k0), dst, wave, lane, j);
        else dma_piece<HN, B_KC, NW>(p.B, p.ldb, p.N, n0 + (POS == 2 ? HN : 0), k0, dst, wave, lane, j);
    };
    auto issue = [&](auto pos_c, int tile, int buf) {
        constexpr int POS = decltype(pos_c)::value;
#pragma unroll
        for (int j = 0; j < ((POS == 0 || POS == 3) ? PA : PB); ++j) issue_piece(pos_c, tile, buf, j);
    };
    bf16x8 fa[FM][BK / 16], fb0[FN][BK / 16], fb1[FN][BK / 16];
    auto read_a = [&](int buf, int half) {
        const unsigned char* T = smem + buf * BUF + half * A_HALF;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk)
#pragma unroll
            for (int f = 0; f < FM; ++f) fa[f][kk] = frag<HM, A_KC>(T, wm * 32 * FM + f * 32, kk, lane);
    };
    auto read_b = [&](int buf, int half, bf16x8 (&fb)[FN][BK / 16]) {
        const unsigned char* T = smem + buf * BUF + 2 * A_HALF + half * B_HALF;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk)
#pragma unroll
            for (int f = 0; f < FN; ++f) fb[f][kk] = frag<HN, B_KC>(T, wn * 32 * FN + f * 32, kk, lane);
    };
    // MFMA slot of one quadrant; the DMA pieces of half-tile POS (k-tile `tile`, buffer `buf`; POS < 0: none) are issued BETWEEN
    // the MFMAs: a piece costs the wave 60-180 clocks of issue, which the matrix pipe spends on the MFMAs already queued —
    // in the load slot the same pieces made that slot (DMA + up to 12 fragment reads) longer than the partner group's 256
    // clocks of MFMA, and the matrix pipe idled at every other barrier (tools/bt_phase_probe.py: 3500 -> clocks per k-tile)
    auto mma = [&](f32x16 (&c)[NACC][NF], bf16x8 (&fb)[FN][BK / 16], auto pos_c, int tile, int buf, int st = -1) {
        constexpr int POS = decltype(pos_c)::value;
        constexpr int NP = POS < 0 ? 0 : (POS == 0 || POS == 3) ? PA : PB, NM = (BK / 16) * NF;
        constexpr int NPD = NP > 0 ? NP : 1, STEP = NM / NPD > 0 ? NM / NPD : 1;
        if (st >= 0) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); stamp(st); }
        if constexpr (ASM_READS) {
            frags_ready();
#pragma unroll
            for (int kk = 0; kk < BK / 16; ++kk) {
#pragma unroll
                for (int f = 0; f < FM; ++f) frag_tie(fa[f][kk]);
#pragma unroll
                for (int f = 0; f < FN; ++f) frag_tie(fb[f][kk]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk)
#pragma unroll
            for (int fm = 0; fm < FM; ++fm)
#pragma unroll
                for (int fn = 0; fn < FN; ++fn) {
                    c[kk % NACC][fm * FN + fn] =
                        __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[fm][kk], fb[fn][kk], c[kk % NACC][fm * FN + fn], 0, 0, 0);
                    if constexpr (NP > 0) {
                        const int m = (kk * FM + fm) * FN + fn;
                        if (m % STEP == 0 && m / STEP < NP) {
                            __builtin_amdgcn_sched_barrier(0);
                            issue_piece(pos_c, tile, buf, m / STEP);
                            if (m / STEP == NP - 1 || m == NM - 1)
                                for (int r = m / STEP + 1; r < NP && m == NM - 1; ++r) issue_piece(pos_c, tile, buf, r);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                }
        __builtin_amdgcn_s_setprio(0);
        if (st >= 0) stamp(st + 1);
    };
    // the barrier that ends a load slot; the MFMA slot of a staggered workgroup ends with a second one
    auto load_done = [&]() { wg_barrier(); };
    auto mma_done = [&]() {
        if constexpr (STAGGER) wg_barrier();
    };
    constexpr int W4 = 2 * (PA + PB);               // DMA instructions of four consecutive half-tiles
    using NoDma = std::integral_constant<int, -1>;

    // one k-tile = four phases.  MODE 0: steady state (k-tiles t + 1 and t + 2 exist); 1: t == nk - 2; 2: t == nk - 1.
    // Issue order of the half-tiles: ... A-lo(t) B-lo(t) B-hi(t) A-hi(t) A-lo(t+1) ...; phase g = 4 t + p issues element g + 6 (in its
    // MFMA slot) and waits (in its load slot, i.e. BEFORE that issue) for element g + 2, which phase g + 1 reads: the three
    // elements g + 3 .. g + 5 stay in flight.
#ifndef VITAE_BT_LMASK
#define VITAE_BT_LMASK 0          // bit p set: the DMA of phase p + 1 is issued in its LOAD slot (before the counted wait), else between
                                  // the MFMAs.  Measured (256x256, clocks per k-tile): 0 (all between the MFMAs) 2880; 8: 3150; 2: 3080; 10: 3370; 15: 3530 — a DMA
                                  // issued by the wave in its load slot stalls the MFMA issue of its SIMD partner (that partner's MFMA slot: 320 -> 560)
#endif
    constexpr bool L1 = VITAE_BT_LMASK & 1, L2 = VITAE_BT_LMASK & 2, L3 = VITAE_BT_LMASK & 4, L4 = VITAE_BT_LMASK & 8;
    constexpr int PB_HI = PB, PA_HI = PA, PA_LO = PA, PB_LO = PB;
    auto ktile = [&](auto mode_c, int t) {
        constexpr int MODE = decltype(mode_c)::value;
        const int buf = t & 1;
        const int sb = (MODE == 0 && p.dbg && t == 2) ? 3 : -100;       // stamps 3..14 in k-tile 2
        // P1: (A-lo, B-lo); issues B-hi(t + 1); needs B-hi(t) for P2: younger A-hi(t), A-lo(t+1), B-lo(t+1) (+ its own)
        if constexpr (MODE <= 1 && L1) issue(std::integral_constant<int, 2>{}, t + 1, buf ^ 1);
        read_a(buf, 0);
        read_b(buf, 0, fb0);
        if constexpr (MODE <= 1) wait_vmcnt<2 * PA + PB + (L1 ? PB_HI : 0)>(); else wait_vmcnt<PA>();
        load_done();
        if constexpr (MODE <= 1 && !L1) mma(acc[0][0], fb0, std::integral_constant<int, 2>{}, t + 1, buf ^ 1, sb);
        else mma(acc[0][0], fb0, NoDma{}, 0, 0, sb);
        mma_done();
        if (sb >= 0) stamp(sb + 2);
        // P2: (A-lo, B-hi); issues A-hi(t + 1); needs A-hi(t) for P3: younger A-lo(t+1), B-lo(t+1), B-hi(t+1) (+ its own)
        if constexpr (MODE <= 1 && L2) issue(std::integral_constant<int, 3>{}, t + 1, buf ^ 1);
        read_b(buf, 1, fb1);
        if constexpr (MODE <= 1) wait_vmcnt<PA + 2 * PB + (L2 ? PA_HI : 0)>(); else wait_vmcnt<0>();
        load_done();
        if constexpr (MODE <= 1 && !L2) mma(acc[0][1], fb1, std::integral_constant<int, 3>{}, t + 1, buf ^ 1, sb + 3);
        else mma(acc[0][1], fb1, NoDma{}, 0, 0, sb + 3);
        mma_done();
        if (sb >= 0) stamp(sb + 5);
        // P3: (A-hi, B-hi); issues A-lo(t + 2); P4 reads nothing
        if constexpr (MODE == 0 && L3) issue(std::integral_constant<int, 0>{}, t + 2, buf);
        read_a(buf, 1);
        load_done();
        if constexpr (MODE == 0 && !L3) mma(acc[1][1], fb1, std::integral_constant<int, 0>{}, t + 2, buf, sb + 6);
        else mma(acc[1][1], fb1, NoDma{}, 0, 0, sb + 6);
        mma_done();
        if (sb >= 0) stamp(sb + 8);
        // P4: (A-hi, B-lo); issues B-lo(t + 2); needs A-lo, B-lo(t+1) for P1: younger B-hi(t+1), A-hi(t+1), A-lo(t+2) (+ its own)
        if constexpr (MODE == 0 && L4) issue(std::integral_constant<int, 1>{}, t + 2, buf);
        if constexpr (MODE == 0) wait_vmcnt<2 * PA + PB + (L4 ? PB_LO : 0)>(); else if constexpr (MODE == 1) wait_vmcnt<PA + PB>();
        load_done();
        if constexpr (MODE == 0 && !L4) mma(acc[1][0], fb0, std::integral_constant<int, 1>{}, t + 2, buf, sb + 9);
        else mma(acc[1][0], fb0, NoDma{}, 0, 0, sb + 9);
        mma_done();
        if (sb >= 0) stamp(sb + 11);
    };

    // prologue: k-tile 0 completely, A-lo and B-lo of k-tile 1
    issue(std::integral_constant<int, 0>{}, 0, 0);
    issue(std::integral_constant<int, 1>{}, 0, 0);
    issue(std::integral_constant<int, 2>{}, 0, 0);
    issue(std::integral_constant<int, 3>{}, 0, 0);
    issue(std::integral_constant<int, 0>{}, 1, 1);
    issue(std::integral_constant<int, 1>{}, 1, 1);
    stamp(1);
    wait_vmcnt<W4>();                               // A-lo(0), B-lo(0) landed
    load_done();
    if (late) load_done();                          // group 1 starts one barrier later
    stamp(2);
#pragma unroll 1
    for (int t = 0; t < nk - 2; ++t) {
        if (t == 2) stamp(15);
        ktile(std::integral_constant<int, 0>{}, t);
    }
    ktile(std::integral_constant<int, 1>{}, nk - 2);
    ktile(std::integral_constant<int, 2>{}, nk - 1);
    stamp(16);
    if (STAGGER && !late) load_done();              // group 0 meets group 1's last barrier

    bt_tail<BM, BN, WM, WN, NACC>(p, acc, smem, m0, n0, tm, tn, zid, wave, lane, stamp);
}

template <int BM, int BN, int WM, int WN, bool A_KC, bool B_KC>
__global__ __launch_bounds__(64 * WM * WN, 2) void gemm_bt_kernel(const GArgs p) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[BtCfg<BM, BN, WM, WN>::SMEM];      // the ONLY LDS object
    gemm_bt_body<BM, BN, WM, WN, A_KC, B_KC>(p, blockIdx.x, blockIdx.z, smem);
}

// a group of weight-gradient problems (BtGroup) as one launch of ping-pong 128x128 tiles
__global__ __launch_bounds__(256, 2) void gemm_bt_wgrad_group_kernel(const BtGroup g) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[BtCfg<128, 128, 2, 2>::SMEM];
    const int b = blockIdx.x;
    const int i = bt_group_index(g, b);
    gemm_bt_body<128, 128, 2, 2, false, false>(g.p[i], b - g.start[i], blockIdx.z, smem);
}

template <int BM, int BN, int WM, int WN>
static void bt_launch_cfg(const GArgs& p, bool a_kc, bool b_kc, hipStream_t st) {
    const dim3 grid(8 * cdiv((long)p.tiles_m * p.tiles_n, 8), 1, p.splits), block(64 * WM * WN);
    if (a_kc && b_kc) hipLaunchKernelGGL((gemm_bt_kernel<BM, BN, WM, WN, true, true>), grid, block, 0, st, p);
    else if (a_kc && !b_kc) hipLaunchKernelGGL((gemm_bt_kernel<BM, BN, WM, WN, true, false>), grid, block, 0, st, p);
    else if (!a_kc && !b_kc) hipLaunchKernelGGL((gemm_bt_kernel<BM, BN, WM, WN, false, false>), grid, block, 0, st, p);
}

bool bt_tile_dims(int id, int& bm, int& bn) {
    switch (id) {
        case 0: bm = 256; bn = 256; return true;
        case 3: bm = 128; bn = 128; return true;
        case 4: bm = 128; bn = 128; return true;       // wave-specialised (4 MFMA waves + 4 DMA waves, one workgroup per CU)
        case 5: bm = 64; bn = 64; return true;         // ... on a 64 x 64 tile (unsplit launches)
        case 6: bm = 128; bn = 256; return true;       // ... on a 128 x 256 tile, weight-gradient form only
        case 7: bm = 128; bn = 64; return true;        // ... on a 128 x 64 tile: the 64 x 64 workgroup with two fragments per wave
        default: return false;
    }
}

// p: a complete problem descriptor (no a_rowsum); tiles_m / tiles_n are set here
int bt_launch(GArgs p, int a_kc, int b_kc, int id, hipStream_t st) {
    int bm, bn;
    if (!bt_tile_dims(id, bm, bn)) return VITAE_ERR_INVALID_ARG;
    if (!p.vec_epi || p.a_rowsum || (p.K % BK) || p.splits < 1) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (!a_kc && b_kc) return VITAE_ERR_UNSUPPORTED_SHAPE;
    // every split gets k_per_split (a multiple of 64) except the last; each needs >= 2 k-tiles
    if (!bt_k_ranges(p.K, 2, p.splits, p.k_per_split)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    p.tiles_m = cdiv(p.M, bm); p.tiles_n = cdiv(p.N, bn);
    if (p.splits > 1 && (!p.ws || id == 0 || (long)p.tiles_m * p.tiles_n > VITAE_GLDS_TICKETS || p.epi == VITAE_EPI_GELU)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    // (128x64 / 64x128 on TWO waves, three workgroups per CU, were tried for the batch-8 encoder shapes where the vendor library uses
    // 128x64 / 128x96 macro tiles: 13.9 vs 13.4 us for the 64-row family on qkv, 15.7 vs 14.4 on fc1 — not kept.)
    // (256x128 and 128x256 on eight waves were built and measured too: four MFMAs per phase against the same barrier / DMA
    // overhead as eight — 2150 clocks per k-tile for 1024 of MFMA — never the best tile on any shape of the step: not kept)
    if (id == 6 && (a_kc || b_kc)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (id == 0) bt_launch_cfg<256, 256, 2, 4>(p, a_kc, b_kc, st);
    else if (id == 4 || id == 6) ws_launch(p, a_kc, b_kc, id, st);
    else if (id == 5 || id == 7) ws64_launch(p, a_kc, b_kc, id, st);
    else bt_launch_cfg<128, 128, 2, 2>(p, a_kc, b_kc, st);
    return vitae_launch_status();
}

// n <= 4 complete weight-gradient descriptors (A = dy16 [K, M] row-contiguous, B = x16 [K, N], same K, vec_epi set); `splits`
// k-ranges for all of them; ws: tickets + partial tiles for the sum of their tiles
int bt_wgrad_group_launch(GArgs* ps, int n, int splits, hipStream_t st, int kind /* 0 ping-pong 128x128, 1 ws 128x128, 2 ws 128x256 */) {
    if (n < 1 || n > 4) return VITAE_ERR_INVALID_ARG;
    BtGroup g;
    int total = 0, tiles = 0;
    const int K = ps[0].K;
    int kps;
    if (!bt_k_ranges(K, 2, splits, kps)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    for (int i = 0; i < 4; ++i) {
        g.start[i] = total;
        if (i >= n) { g.p[i] = g.p[0]; continue; }
        GArgs& p = ps[i];
        if (!p.vec_epi || p.a_rowsum || p.K != K || (K % BK)) return VITAE_ERR_UNSUPPORTED_SHAPE;
        p.k_per_split = kps; p.splits = splits;
        p.tiles_m = cdiv(p.M, 128); p.tiles_n = cdiv(p.N, kind == 2 ? 256 : 128);
        p.tile0 = tiles;
        tiles += p.tiles_m * p.tiles_n;
        total += 8 * cdiv(p.tiles_m * p.tiles_n, 8);
        g.p[i] = p;
    }
    g.start[4] = total;
    for (int i = n; i < 4; ++i) g.start[i] = total;
    if (splits > 1 && (!ps[0].ws || tiles > VITAE_GLDS_TICKETS)) return VITAE_ERR_UNSUPPORTED_SHAPE;
    if (kind == 1 || kind == 2) ws_wgrad_group_launch(g, total, splits, kind, st);
    else hipLaunchKernelGGL(gemm_bt_wgrad_group_kernel, dim3(total, 1, splits), dim3(256), 0, st, g);
    return vitae_launch_status();
}

}  // namespace vglds
