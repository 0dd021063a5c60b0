// What the big-tile and wave-specialised bf16 GEMM families share.  One translation unit per family:
//   gemm_bt.hip     ping-pong 256x256 / 128x128 tiles (ids 0, 3), their grouped weight-gradient kernel, and the dispatchers
//   gemm_ws.hip     wave-specialised 128x128 / 128x256 tiles (ids 4, 6) and their grouped weight-gradient kernels
//   gemm_ws64.hip   wave-specialised 64x64 tile (id 5) and 128x64 tile (id 7), the two-plane form and the paired dgrad + wgrad launch
//   gemm_wsx3.hip   fp32x3 on the 64x64 structure
// Here: the barrier and counted waits of the producer / consumer protocol, the wave-private epilogue and the family's tail
// (bt_tail), the 64x64 consumer loop, the host-side k-range rule, and the per-family launch entry points the dispatchers of
// gemm_bt.hip call.
// Every piece here was checked per kernel with tools/isa_report.py (profiles/split_gemm_bt_isa.txt): same registers, spills, LDS
// and scratch, and no vector, MFMA, LDS or buffer instruction more or fewer than with the piece written out.  Pieces that did
// not pass stay written out where they are used: the tile decode (below), the 64x64 tail in gemm_ws64_body and gemm_wsx3_body
// (note there), and the DMA producer protocol of the three wave-specialised bodies (kept as copies: its three forms differ in
// stamps and in gemm_ws_body's `active` predicate).
#pragma once
#include <cstdlib>
#include <type_traits>
#include "glds_gemm.hpp"

namespace vglds {

// k-slice indices of a 64-deep k-tile as types (the fragment readers take them as template values)
using K0 = std::integral_constant<int, 0>; using K1 = std::integral_constant<int, 1>;
using K2 = std::integral_constant<int, 2>; using K3 = std::integral_constant<int, 3>;

// a workgroup barrier the compiler moves nothing across
__device__ __forceinline__ void wg_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// XCD-aware AND balanced tile map (block b runs on XCD b % 8): the T = tiles_m * tiles_n tiles are cut into eight contiguous
// chunks of the linear order (sizes differ by at most one), XCD x takes chunk x.  The linear order walks the SHORTER operand's
// tiles fastest, so a chunk covers whole column tiles (all row tiles under them) — or whole row tiles when A is the larger
// operand (by_rows): an XCD's L2 holds 1/8 of one operand and streams the other.  (The 64-row kernels give XCD x the column
// tiles x, x + 8, ...: with 18 column tiles two XCDs get three columns and six get two — a 1.5x longer tail.)
// The grid has 8 * ceil(T / 8) blocks; the padding blocks leave at once.
// The decode is WRITTEN OUT at the top of each of the five bodies (T, xq, xr, xcd, lin, early return, tn, tm), not a function: as a
// function returning (live, tm, tn) hipcc moved the two divisions in front of the padding blocks' exit and, in the 64x64 bodies, in
// front of the first DMA (the stand-alone 64x64 launches measured 0.2-0.4 us slower, the batch-4 step 0.3 %); with the exit inside
// the function other kernels changed registers and vector instructions (tools/isa_report.py).

// Producer side of the S-stage pipeline (PT DMA instructions per wave and k-tile): all but the youngest `fly` tiles of this wave's
// pieces have landed.  At most S - 2 tiles stay in flight behind the one waited for.
template <int S, int PT> __device__ __forceinline__ void wait_tiles(const int fly) {
    if (S >= 5 && fly >= 3) wait_vmcnt<(S >= 5 ? 3 : 1) * PT>();
    else if (S >= 4 && fly >= 2) wait_vmcnt<(S >= 4 ? 2 : 1) * PT>();
    else if (fly >= 1) wait_vmcnt<PT>();
    else wait_vmcnt<0>();
}

// Host: cut K into `splits` k-ranges.  Every range gets kps (a multiple of 64) except the last, and `splits` drops to the number
// of ranges that are not empty.  false: some range is shorter than min_tiles k-tiles (the k-loops need their prologue depth).
static inline bool bt_k_ranges(const int K, const int min_tiles, int& splits, int& kps) {
    kps = cdiv(cdiv(K, splits), BK) * BK;
    splits = cdiv(K, kps);
    return kps >= min_tiles * BK && K - (splits - 1) * kps >= min_tiles * BK;
}

// Two-plane weights on every tile (round 5): B = [W hi | W lo] side by side ([N, 2 Ka]) and the reduction runs over 2 Ka with the A
// operand (k-contiguous, Ka wide) WRAPPING — k-tile t of the second half re-reads the activations of k-tile t - Ka / 64:
// y = x16 Whi^T + x16 Wlo^T out of one unmodified k-loop.  p.a_kwrap = Ka (a multiple of 64; 0 = no wrap).
__device__ __forceinline__ int a_wrap(const GArgs& p, int k0) { return (p.a_kwrap && k0 >= p.a_kwrap) ? k0 - p.a_kwrap : k0; }

template <int BM, int BN, int WM, int WN> struct BtCfg {
    static constexpr int NW = WM * WN, NT = 64 * NW;
    static constexpr int HM = BM / 2, HN = BN / 2;                          // rows of a half-tile
    static constexpr int FM = HM / (32 * WM), FN = HN / (32 * WN);          // 32x32 fragments of a wave inside one half
    static constexpr int A_HALF = HM * BK * 2, B_HALF = HN * BK * 2;        // bytes
    static constexpr int BUF = 2 * A_HALF + 2 * B_HALF, SMEM = 2 * BUF;
    static_assert(FM >= 1 && FN >= 1 && HM == 32 * WM * FM && HN == 32 * WN * FN, "wave arrangement does not tile the halves");
};

// Epilogue of ONE wave's part of a quadrant ((32 FM) x (32 FN) outputs), WAVE-PRIVATE: the wave parks its fragments in its own LDS
// region (Tw, row stride 32 FN floats: conflict-free for the ds_write_b32 of the MFMA layout — 32 consecutive columns per half
// wave — and for the ds_read_b128 lane groups of the row-major read-back), and re-reads them row-major: 8 FN lanes own one row
// (four consecutive columns each), so C, the bf16 copy, aux, residual and the old C move 16 bytes per lane in whole 128-byte
// (FN = 1) lines.  No workgroup barrier anywhere: a wave's LDS operations execute in order, and nobody else touches Tw.
// History (tools/bt_phase_probe.py, 256x256 tile, clocks per quadrant): workgroup-wide staging with every epilogue kind behind
// run-time branches: park 1900 + rows 5800 (5100 with the global stores removed: instruction-latency bound); specialised on the
// epilogue kind / full tiles: 1900 + 3200; wave-private: see DESIGN.md.
// KIND: which epilogue (one instantiation each, so that NO load in the row loop sits behind a run-time condition: hipcc waits
// vmcnt(0) in front of every conditionally executed load, and on gfx9 that also waits for every global store issued before —
// the first version spent ~4000 clocks per quadrant waiting for its own stores):
//   0 plain (bias), 1 + residual, 2 + old C (accumulate), 3 GELU (aux <- pre-activation), 4 GELU' (aux read), 5 ReLU mask (aux
//   read), 6 ReLU, 7 anything else (every option behind run-time checks: correct, slow).
// All global loads of the wave's part (one 16-byte load per row pass) are issued BEFORE the first store.
// AUX16 (kinds 3 / 4 / 5 / 7): the aux array holds bf16.  A template parameter, not a run-time test: with `if (p.aux16)` around the
// aux loads hipcc put every one of them behind a branch and an `s_waitcnt vmcnt(0)` — eight serialised memory round trips per
// quadrant in the GELU' epilogue (round 4, ISA of gemm_bt_kernel<256, 256, 2, 4, true, false>).
template <int FM, int FN, int KIND, bool FULL, bool AUX16>
__device__ __forceinline__ void bt_wave_rows(const GArgs& p, int mb, int nb, const float* Tw, int lane, float& sqs, f32x4& csum, const f32x4 bias4) {
    constexpr int S = 32 * FN, LPR = 8 * FN, RPI = 64 / LPR, PASSES = 32 * FM / RPI, PB = PASSES >= 4 ? 4 : PASSES;
    const int cg = lane % LPR, rr = lane / LPR;
    const int n = nb + 4 * cg;
    const bool ncol = FULL || n < p.N;
    const int nc = ncol ? n : 0;
    const int ldaux = (int)p.ldaux, ldr = (int)p.ldr, ldc = (int)p.ldc, ldc16 = (int)p.ldc16;
    const int epi = KIND == 7 ? p.epi : KIND == 3 ? VITAE_EPI_GELU : KIND == 4 ? VITAE_EPI_DGELU : KIND == 5 ? VITAE_EPI_RELU_MASK
                  : KIND == 6 ? VITAE_EPI_RELU : VITAE_EPI_NONE;
    const bool need_aux = KIND == 7 ? (p.epi == VITAE_EPI_DGELU || p.epi == VITAE_EPI_RELU_MASK) : (KIND == 4 || KIND == 5);
    const bool has_res = KIND == 7 ? p.residual != nullptr : KIND == 1;
    const bool acc_c = KIND == 7 ? (p.C && p.accumulate) : KIND == 2;
    // one array per operand kind; an instantiation other than 7 uses at most one of them (and loads all its passes up front;
    // kind 7 loads batch by batch: three arrays of all passes would spill next to 128 live accumulators)
    constexpr int LDN = KIND == 7 ? PB : PASSES;
    f32x4 ax[AUX16 ? 1 : LDN], rs[LDN], co[LDN];
    bf16x4 ax16[AUX16 ? LDN : 1];                  // raw: converted where it is used, so that the loads of a batch fly together
    auto load_ops = [&](int q0) {
#pragma unroll
        for (int q = 0; q < LDN; ++q) {
            const int mr = mb + rr + (q0 + q) * RPI;
            const int mc = FULL ? mr : min(mr, p.M - 1);
            if (need_aux) {
                if constexpr (AUX16) ax16[q] = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(p.aux) + mc * ldaux + nc);
                else ax[q] = *reinterpret_cast<const f32x4*>(p.aux + mc * ldaux + nc);
            }
            if (has_res) rs[q] = *reinterpret_cast<const f32x4*>(p.residual + mc * ldr + nc);
            if (acc_c) co[q] = *reinterpret_cast<const f32x4*>(p.C + mc * ldc + nc);
        }
    };
    if constexpr (KIND != 7) load_ops(0);
    const float* Trow = Tw + rr * S + 4 * cg;
    // LDS reads ahead of the first store: the whole part when it is four passes, else batch by batch (eight passes of x next to
    // the 128 live accumulators of the 256x256 tile spill)
    constexpr bool XALL = PASSES <= 4;
    f32x4 x[XALL ? PASSES : PB];
    if constexpr (XALL) {
#pragma unroll
        for (int q = 0; q < PASSES; ++q) x[q] = *reinterpret_cast<const f32x4*>(Trow + q * RPI * S);
    }
#pragma unroll
    for (int pb = 0; pb < PASSES; pb += PB) {
        if constexpr (KIND == 7) load_ops(pb);
        constexpr int LB = KIND == 7 ? 0 : 1;      // index of this batch's first pass in the operand arrays: pb * LB
        constexpr int XB = XALL ? 1 : 0;
        if constexpr (!XALL) {
#pragma unroll
            for (int q = 0; q < PB; ++q) x[q] = *reinterpret_cast<const f32x4*>(Trow + (pb + q) * RPI * S);
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) {
            const int m = mb + rr + (pb + q) * RPI;
            const bool ok = FULL || (ncol && m < p.M);
            f32x4 v = x[pb * XB + q];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += bias4[e];
            f32x4 axv = {0.f, 0.f, 0.f, 0.f};
            if (need_aux) {
                if constexpr (AUX16) {
                    const bf16x4 h = ax16[pb * LB + q];
                    axv = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
                } else {
                    axv = ax[pb * LB + q];
                }
            }
            if (epi == VITAE_EPI_GELU) {
                f32x4 y, dy;
                if (p.exact) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { float ye, de; gelu_erf_both(v[e], ye, de); y[e] = ye; dy[e] = de; }
                } else {
                    gelu_fast4(v, y, dy);
                }
                const f32x4 sv = p.auxd ? dy : v;                // what the backward gets: GELU'(x) (VITAE_EPI_AUX_DERIV) or x itself
                if (ok) {
                    if constexpr (AUX16) {
                        bf16x4 h;
#pragma unroll
                        for (int e = 0; e < 4; ++e) h[e] = (__bf16)sv[e];
                        *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(p.aux) + m * ldaux + n) = h;
                    } else {
                        *reinterpret_cast<f32x4*>(p.aux + m * ldaux + n) = sv;
                    }
                }
                v = y;
            } else if (epi == VITAE_EPI_DGELU) {
                f32x4 g = axv;                                   // (aux already holds the derivative: a multiply)
                if (!p.auxd) {
                    if (p.exact) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) g[e] = gelu_erf_grad(axv[e]);
                    } else {
                        g = gelu_fast_grad4(axv);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] *= g[e];
            } else if (epi == VITAE_EPI_RELU_MASK) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = axv[e] > 0.f ? v[e] : 0.f;
            } else if (epi == VITAE_EPI_RELU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            }
            if (has_res) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += rs[pb * LB + q][e];
            }
            if (acc_c) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += co[pb * LB + q][e];
            }
            if (ok) {
                if (p.C) *reinterpret_cast<f32x4*>(p.C + m * ldc + n) = v;
                if (p.C16) {
                    bf16x4 v16;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v16[e] = (__bf16)v[e];
                    *reinterpret_cast<bf16x4*>(p.C16 + m * ldc16 + n) = v16;
                }
                if (p.out_colsum) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) csum[e] += v[e];
                }
                if (p.sqacc) sqs += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
            }
        }
    }
}

__device__ __forceinline__ int bt_epilogue_kind(const GArgs& p) {
    const bool res = p.residual != nullptr, accc = p.C && p.accumulate;
    if (p.epi == VITAE_EPI_NONE) return res && accc ? 7 : res ? 1 : accc ? 2 : 0;
    if (res || accc) return 7;
    return p.epi == VITAE_EPI_GELU ? 3 : p.epi == VITAE_EPI_DGELU ? 4 : p.epi == VITAE_EPI_RELU_MASK ? 5 : p.epi == VITAE_EPI_RELU ? 6 : 7;
}

// Which of the specialised instantiations above a kernel carries (KINDS of bt_wave_epilogue): bit k = kind k (0 - 6; for 3 / 4 / 5
// with an fp32 aux), bit 8 + k = kind k with a bf16 aux (3 / 4 / 5).  Kind 7 is in every set and takes whatever the set leaves out:
// a caller outside a kernel's set gets the same result from the run-time-checked path, only slower.  One instantiation is 5-6 KB
// of code on a 32 x 32 part and 10-12 KB on a 64 x 32 part, a workgroup runs ONE of them, and the full set was 125 of the 132 KB of a
// 64 x 64 kernel: the sets below are what the library's callers launch in each operand form.
constexpr int bt_kind(int k) { return 1 << k; }
constexpr int bt_kind16(int k) { return 1 << (8 + k); }
constexpr int BT_KINDS_ALL = 0x7f | bt_kind16(3) | bt_kind16(4) | bt_kind16(5);
// forward form (x W^T): everything but the two epilogues that read what a forward saved
constexpr int BT_KINDS_FWD = BT_KINDS_ALL & ~(bt_kind(4) | bt_kind16(4) | bt_kind(5) | bt_kind16(5));
// input-gradient form (dy W): plain, accumulate into dx, GELU' from either aux type
constexpr int BT_KINDS_DGRAD = bt_kind(0) | bt_kind(2) | bt_kind(4) | bt_kind16(4);
// weight-gradient form (dy^T x): plain, accumulate into dW
constexpr int BT_KINDS_WGRAD = bt_kind(0) | bt_kind(2);

// csum: the column sums of this part are ADDED to it (lane layout: the four columns nb + 4 (lane % (8 FN)) ..., one partial per row
// group).  defer_colsum: nothing is flushed — the caller folds the parts of a whole workgroup tile and issues ONE atomic per column
// (bt_tail); otherwise the wave folds its own row groups and adds its sums to p.out_colsum itself (csum should come in as zero).
template <int FM, int FN, int KINDS = BT_KINDS_ALL>
__device__ __forceinline__ void bt_wave_epilogue(const GArgs& p, int kind, int mb, int nb, const float* Tw, int lane, float& sqs, const f32x4 bias4,
                                                 f32x4& csum, const bool defer_colsum) {
    constexpr int LPR = 8 * FN;
    const bool full = mb + 32 * FM <= p.M && nb + 32 * FN <= p.N;
    if constexpr (KINDS != BT_KINDS_ALL) {         // (wave-uniform; with the full set the switch is what it always was)
        const int bit = kind + ((kind >= 3 && kind <= 5 && p.aux16) ? 8 : 0);
        if (kind > 6 || !((KINDS >> bit) & 1)) kind = 7;
    }
#define VITAE_BT_ROWS(E)                                                                       \
    case E:                                                                                    \
        if constexpr ((KINDS & bt_kind(E)) != 0) {                                             \
            if (full) bt_wave_rows<FM, FN, E, true, false>(p, mb, nb, Tw, lane, sqs, csum, bias4);  \
            else bt_wave_rows<FM, FN, E, false, false>(p, mb, nb, Tw, lane, sqs, csum, bias4);      \
        }                                                                                      \
        break;
#define VITAE_BT_ROWS_AUX(E)                                                                   \
    case E:                                                                                    \
        if (p.aux16) {                                                                         \
            if constexpr ((KINDS & bt_kind16(E)) != 0) {                                       \
                if (full) bt_wave_rows<FM, FN, E, true, true>(p, mb, nb, Tw, lane, sqs, csum, bias4);  \
                else bt_wave_rows<FM, FN, E, false, true>(p, mb, nb, Tw, lane, sqs, csum, bias4);      \
            }                                                                                  \
        } else {                                                                               \
            if constexpr ((KINDS & bt_kind(E)) != 0) {                                         \
                if (full) bt_wave_rows<FM, FN, E, true, false>(p, mb, nb, Tw, lane, sqs, csum, bias4); \
                else bt_wave_rows<FM, FN, E, false, false>(p, mb, nb, Tw, lane, sqs, csum, bias4);     \
            }                                                                                  \
        }                                                                                      \
        break;
    switch (kind) {
        VITAE_BT_ROWS(0) VITAE_BT_ROWS(1) VITAE_BT_ROWS(2) VITAE_BT_ROWS_AUX(3) VITAE_BT_ROWS_AUX(4) VITAE_BT_ROWS_AUX(5) VITAE_BT_ROWS(6)
        default:
            if (p.aux16) bt_wave_rows<FM, FN, 7, false, true>(p, mb, nb, Tw, lane, sqs, csum, bias4);
            else bt_wave_rows<FM, FN, 7, false, false>(p, mb, nb, Tw, lane, sqs, csum, bias4);
            break;
    }
#undef VITAE_BT_ROWS
#undef VITAE_BT_ROWS_AUX
    if (defer_colsum) return;                      // (the caller folds csum over its parts: by reference, never through a pointer — that put it in scratch)
    if (p.out_colsum) {
        // lanes with equal (lane % LPR) hold the same four columns: fold the row groups, then one atomic per column
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int d = LPR; d < 64; d <<= 1) csum[e] += __shfl_xor(csum[e], d, 64);
        const int n = nb + 4 * (lane % LPR);
        if (lane < LPR && n < p.N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) atomicAdd(p.out_colsum + n + e, csum[e]);
        }
    }
}

// the fragments of one quadrant -> the wave's own LDS region
template <int FM, int FN, int NACC>
__device__ __forceinline__ void bt_park_quadrant(const f32x16 (&acc)[NACC][FM * FN], int lane, float* Tw) {
    constexpr int S = 32 * FN;
    const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int fm = 0; fm < FM; ++fm)
#pragma unroll
        for (int fn = 0; fn < FN; ++fn)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[0][fm * FN + fn][r];
                if (NACC == 2) v += acc[NACC - 1][fm * FN + fn][r];
                Tw[(fm * 32 + crow(r, hi)) * S + fn * 32 + l31] = v;
            }
}

// What follows the k-loop of a big-tile workgroup: the in-launch split-K fix-up (tiles below 256 x 256) and the wave-private
// epilogue, quadrant by quadrant.  `wave` / threadIdx.x index the NW = WM * WN waves that hold accumulators (the wave-specialised
// kernel's producer waves have left by now: a barrier only counts the waves still alive).
template <int BM, int BN, int WM, int WN, int NACC, class Stamp>
__device__ __forceinline__ void bt_tail(const GArgs& p, f32x16 (&acc)[2][2][NACC][BtCfg<BM, BN, WM, WN>::FM * BtCfg<BM, BN, WM, WN>::FN],
                                        unsigned char* smem, const int m0, const int n0, const int tm, const int tn, const int zid,
                                        const int wave, const int lane, Stamp stamp) {
    using Cf = BtCfg<BM, BN, WM, WN>;
    constexpr int NW = Cf::NW, HM = Cf::HM, HN = Cf::HN, FM = Cf::FM, FN = Cf::FN, NF = FM * FN;
    const int wm = wave / WN, wn = wave % WN;
    // epilogue: every wave on its own, quadrant by quadrant through its own 32 FM x 32 FN floats of LDS (the stages are free once
    // everybody has left the k-loop).  The loop over quadrants is ROLLED; only the register -> LDS part depends on which
    // accumulators are meant.
    constexpr int TW = 32 * FM * 32 * FN;          // floats per wave
    static_assert(NW * TW * 4 + 64 <= Cf::SMEM, "wave-private staging (+ the norm share of each wave) fits the operand stages");
    float* Tw = reinterpret_cast<float*>(smem) + wave * TW;
    float sqs = 0.f;
    const int kind = bt_epilogue_kind(p);
    if constexpr (BM * BN < 256 * 256) if (p.splits > 1) {     // (the 256x256 tile: 256 KB of partials per split and workgroup - not offered)
        // Split-K inside the launch: every split parks its partial tile in the workspace (fragment order: 16 bytes per lane,
        // lane-contiguous, WRITE-THROUGH stores — sc1 — so the data is on the memory side of the eight L2s without a release
        // fence), drains, takes a ticket; the LAST arriver of a tile re-reads all partials with sc1 loads in split order
        // (bitwise reproducible whatever the arrival order) and runs the epilogue.  cdna_hip_programming.md §6 Guideline 16 R1.
        constexpr int NT = 64 * NW, GROUPS = 4 * NF * 4;                  // 16-byte groups per lane: quadrants x fragments x 4
        const int tile = p.tile0 + tm * p.tiles_n + tn;
        float* part = p.ws + VITAE_GLDS_TICKETS + (long)tile * p.splits * (NT * GROUPS * 4);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(part, 0, p.splits * (NT * GROUPS * 16), 0x00020000);
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const int toff = (int)threadIdx.x * 16;
        if constexpr (NACC == 2) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int f = 0; f < NF; ++f)
#pragma unroll
                        for (int i = 0; i < 16; ++i) acc[a][b][0][f][i] += acc[a][b][NACC - 1][f][i];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc[a][b][0][f][4 * g + e];
                        const int grp = ((a * 2 + b) * NF + f) * 4 + g;
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (zid * GROUPS + grp) * (NT * 16) + toff, 0, 16);
                    }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains its own stores
        __syncthreads();
        int* flag = reinterpret_cast<int*>(smem);
        if (threadIdx.x == 0) *flag = __hip_atomic_fetch_add(reinterpret_cast<int*>(p.ws) + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*flag != p.splits - 1) return;
        __syncthreads();                                          // everyone has read the flag before the staging area is reused
        // all GROUPS loads of one split in flight together (a first version with one quadrant's four at a time cost the last
        // arriver 4 x splits dependent round trips to the memory side, ~1 us each)
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int f = 0; f < NF; ++f)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        acc[a][b][0][f][i] = 0.f;
                        if (NACC == 2) acc[a][b][NACC - 1][f][i] = 0.f;
                    }
#pragma unroll 1
        for (int sp = 0; sp < p.splits; ++sp) {
            f32x4 v[GROUPS];
#pragma unroll
            for (int i = 0; i < GROUPS; ++i)
                v[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (sp * GROUPS + i) * (NT * 16) + toff, 0, 16));
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int f = 0; f < NF; ++f)
#pragma unroll
                        for (int g = 0; g < 4; ++g)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[a][b][0][f][4 * g + e] += v[((a * 2 + b) * NF + f) * 4 + g][e];
        }
        if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<int*>(p.ws) + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
    // the bias of the wave's two column ranges, fetched under the barrier (issued inside the quadrant loop it cost every
    // quadrant one exposed memory latency)
    f32x4 biasq[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int n = n0 + b * HN + wn * 32 * FN + 4 * (lane % (8 * FN));
        biasq[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p.bias && n < p.N) biasq[b] = *reinterpret_cast<const f32x4*>(p.bias + n);
    }
    __syncthreads();                               // every wave is done with the operand stages
    stamp(17);
    float* cred = reinterpret_cast<float*>(smem) + NW * TW + 16;              // column-sum partials [2 A-halves x WM][2 B-halves][HN]
    static_assert((NW * TW + 16 + 4 * WM * HN) * 4 <= Cf::SMEM, "column-sum staging fits behind the wave-private regions");
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        switch (q) {
            case 0: bt_park_quadrant<FM, FN, NACC>(acc[0][0], lane, Tw); break;
            case 1: bt_park_quadrant<FM, FN, NACC>(acc[0][1], lane, Tw); break;
            case 2: bt_park_quadrant<FM, FN, NACC>(acc[1][0], lane, Tw); break;
            default: bt_park_quadrant<FM, FN, NACC>(acc[1][1], lane, Tw); break;
        }
        __builtin_amdgcn_wave_barrier();           // compiler-only: the lanes' writes stay in front of the other lanes' reads
        f32x4 cs = {0.f, 0.f, 0.f, 0.f};
        bt_wave_epilogue<FM, FN>(p, kind, m0 + (q >> 1) * HM + wm * 32 * FM, n0 + (q & 1) * HN + wn * 32 * FN, Tw, lane, sqs, (q & 1) ? biasq[1] : biasq[0],
                                 cs, true);
        if (p.out_colsum) {
            // this quadrant's column sums, folded over the wave's row groups, parked per (A-half, wave row): nothing is carried in
            // registers across the quadrants (eight more live VGPRs spilled next to the 128 accumulators of the 256 x 256 tile)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int d = 8 * FN; d < 64; d <<= 1) cs[e] += __shfl_xor(cs[e], d, 64);
            if (lane < 8 * FN) *reinterpret_cast<f32x4*>(cred + (((q >> 1) * WM + wm) * 2 + (q & 1)) * HN + wn * 32 * FN + 4 * lane) = cs;
        }
        __builtin_amdgcn_wave_barrier();
        stamp(18 + q);
    }
    if (p.out_colsum) {
        // Column sums of the stored tile (the bias gradient of the Linear in front): the 2 WM parked partials of every column are
        // added and ONE value per column and workgroup goes to memory.  (Round 5: one atomic per wave, quadrant and column — 2048
        // per 256 x 256 tile — cost the fc2 input-gradient launches of a batch-32 step 5-10 us each, tools/epi_ablate.py.)
        __syncthreads();
        for (int j = threadIdx.x; j < 2 * HN; j += 64 * NW) {
            const int b = j / HN, c = j % HN, n = n0 + b * HN + c;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < 2 * WM; ++w) t += cred[(w * 2 + b) * HN + c];
            if (n < p.N) atomicAdd(p.out_colsum + n, t);
        }
        __syncthreads();                            // (the norm share below reuses words in front)
    }
    if (p.sqacc) {
        // ONE double atomic per workgroup: every launch of a step adds to the same address, and the L2 serialises them — with one
        // per wave a 700-workgroup launch queued 2800 of them (the ws64 pair launches: 27 us instead of 17 inside the step)
        sqs = wave_sum(sqs);
        float* red = reinterpret_cast<float*>(smem) + NW * TW;
        if (lane == 0) red[wave] = sqs;
        __syncthreads();
        if (threadIdx.x == 0) {
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) tot += red[w];
            atomicAdd(sq_slot(p), (double)tot);
        }
    }
    if (p.dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamp(25); }
}

// What a workgroup needs before its first DMA can leave (tile decoding + operand addressing).  The stand-alone kernels take these as
// LEADING SCALAR kernel arguments: with -amdgpu-kernarg-preload-count=16 they arrive in SGPRs with the dispatch, while the by-value
// descriptor behind them is fetched by scalar loads that nothing on the producers' path waits for (round 6).
struct WsHot {
    const __bf16* A; const __bf16* B; const __bf16* B2;        // (B2: the lo plane of a two-plane weight, else unused)
    int lda, ldb, M, N, K, tiles_m, tiles_n, xcd_m, kps;      // xcd_m: bit 0 the XCD map, bit 1 "p.dbg is set"
};
// the stand-alone kernels' leading scalars (13 dwords; 14 can be preloaded): the tile counts follow from M and N (64 x 64 tiles)
#define WS_HOT_PARAMS const __bf16* A, const __bf16* B, const __bf16* B2, int lda, int ldb, int M, int N, int K, int xcd_m, int kps
#define WS_HOT_FROM_PARAMS WsHot{A, B, B2, lda, ldb, M, N, K, (M + 63) >> 6, (N + 63) >> 6, xcd_m, kps}
#define WS_HOT_ARGS(p) (p).A, (p).B, (p).B2, (int)(p).lda, (int)(p).ldb, (p).M, (p).N, (p).K, (p).xcd_m | ((p).dbg ? 2 : 0), (p).k_per_split

// Up to four weight-gradient problems dW_i[N_i, K_i] (+)= dy_i^T x_i of one transformer block (same reduction length: the padded
// token count) as ONE launch of 128x128 tiles: together they have enough tiles that the reduction needs no split (batch 32
// encoder: 432 tiles) or a split of two (decoder: 192) where each of them alone wanted 3-8 — and the in-launch split-K fix-up was
// half of those launches (tools/wgrad_split_sweep.py).  Block ranges start at multiples of 8: every problem keeps its XCD map.
struct BtGroup { GArgs p[4]; int start[5]; };
// which problem of the group block b belongs to
__device__ __forceinline__ int bt_group_index(const BtGroup& g, const int b) { return (b >= g.start[1]) + (b >= g.start[2]) + (b >= g.start[3]); }

// ---- the four consumer waves of a 64 x 64 workgroup (gemm_ws64.hip, gemm_wsx3.hip): one 32 x 32 fragment per wave --------------
// k-loop: ONE workgroup barrier per k-tile, crossed in the MIDDLE of it.  B_0 is behind the caller; B_{t+1} promises that tile
// t + 1 has landed and lets the producers restage tile t's slot, so every read of tile t is retired (lgkmcnt(0)) in front of it.
// The fragments of slices 0-1 of tile t + 1 are read right behind the barrier, under the MFMAs of slices 2-3 of tile t.
//   rd(base, Kk): the LDS reads of k-slice k of the tile at `base`; mm(Kk): its MFMAs; LG: the lgkmcnt that leaves only the reads of
//   slices 2-3 in flight; k-tile t is in stage t % S, STG bytes each.
template <int LG, int S, int STG, class Rd, class Mm>
__device__ __forceinline__ void ws64_consume(const unsigned char* smem, const int nk, Rd rd, Mm mm) {
    rd(smem, K0{}); rd(smem, K1{});
    int stage = 0;
#pragma unroll 1
    for (int t = 0; t < nk; ++t) {
        const unsigned char* TA = smem + stage * STG;
        __builtin_amdgcn_sched_barrier(0);
        rd(TA, K2{}); rd(TA, K3{});
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(LG) : "memory");      // slices 0-1 are in registers
        __builtin_amdgcn_sched_barrier(0);
        mm(K0{}); mm(K1{});
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               // every read of tile t has retired
        if (t + 1 < nk) {
            wg_barrier();                                                // B_{t+1}
            stage = stage + 1 == S ? 0 : stage + 1;
            const unsigned char* TN = smem + stage * STG;
            rd(TN, K0{}); rd(TN, K1{});
            __builtin_amdgcn_sched_barrier(0);
        }
        mm(K2{}); mm(K3{});
    }
}

// ---- one launch function per family, called by the dispatchers of gemm_bt.hip (the public entry points are in glds_gemm.hpp) ----
// p: the descriptor as bt_launch / bt_wgrad_group_launch completed it (k-ranges, tile counts).
void ws_launch(const GArgs& p, int a_kc, int b_kc, int id /* 4: 128x128, 6: 128x256 (weight-gradient form) */, hipStream_t st);       // gemm_ws.hip
void ws_wgrad_group_launch(const BtGroup& g, int total, int splits, int kind /* 1: 128x128, 2: 128x256 */, hipStream_t st);             // gemm_ws.hip
void ws64_launch(const GArgs& p, int a_kc, int b_kc, int id /* 5: 64x64, 7: 128x64 */, hipStream_t st);                                  // gemm_ws64.hip

}  // namespace vglds
