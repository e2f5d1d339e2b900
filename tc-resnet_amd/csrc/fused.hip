// Whole-network eval-mode forward of TC-ResNet in ONE persistent kernel: a workgroup pulls a group of G
// utterances, keeps every activation of the group in LDS (three rotating buffers), and walks the layer table:
//   features -> conv0 -> [down | conv_a -> conv_b (+shortcut, ReLU)] x blocks -> avg-pool -> fc / fc2 -> softmax.
// (audio_nets/tc_resnet.py:6-54 + slim.softmax, factory/audio_nets.py:147-156, with BN folded to scale/shift.)
//
// Why: the per-layer kernels move ~85 KB of activations per utterance through L2/HBM and pay a pipeline
// fill/drain per launch; fused, the only global traffic is the 9 KB feature tile in and 14 floats out, and the
// weights (258 KB for TCResNet8-1.0) stream from L2 with a register lookahead.  Every convolution is an implicit
// GEMM on the exact-f32 16x16x4 MFMA (bitwise an fmaf chain): D[co][position] with positions = G * T_out packed
// across utterances, A = weights straight from L1/L2, B = activations from the LDS rows (taps, stride and SAME
// padding are plain offsets into the zero-halo rows).  A job is (16 output channels) x (32 positions); the four
// waves of the workgroup take jobs round-robin, one s_barrier per layer.
#include <cstdint>

#include "kernels.h"

namespace tcr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// 16 / 8 bytes per lane through a buffer descriptor (buffer_load_dwordx4 / dwordx2: gfx950_isa.h, buf_load_f32); a compiler without
// the wide builtins takes the same bytes dword by dword.
__device__ __forceinline__ f32x4 buf_load_f32x4(buf_rsrc rs, unsigned lane_off_bytes, unsigned uniform_off_bytes) {
#if __has_builtin(__builtin_amdgcn_raw_buffer_load_b128)
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)lane_off_bytes, (int)uniform_off_bytes, 0));
#else
    return (f32x4){buf_load_f32(rs, lane_off_bytes, uniform_off_bytes), buf_load_f32(rs, lane_off_bytes, uniform_off_bytes + 4u),
                   buf_load_f32(rs, lane_off_bytes, uniform_off_bytes + 8u), buf_load_f32(rs, lane_off_bytes, uniform_off_bytes + 12u)};
#endif
}
__device__ __forceinline__ f32x2 buf_load_f32x2(buf_rsrc rs, unsigned lane_off_bytes, unsigned uniform_off_bytes) {
#if __has_builtin(__builtin_amdgcn_raw_buffer_load_b64)
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)lane_off_bytes, (int)uniform_off_bytes, 0));
#else
    return (f32x2){buf_load_f32(rs, lane_off_bytes, uniform_off_bytes), buf_load_f32(rs, lane_off_bytes, uniform_off_bytes + 4u)};
#endif
}

// Fragments of channel quads [C0, C0 + N) of one tap out of the frozen table's weight image (kernels.h "weight image"): `uni` is the
// byte offset of the tap's first fragment -- layer, row tile, tap: wave-uniform --, `lane` the lane index; a group of four quads is
// [lane][4], so an aligned run of 4 / 2 quads is one 16 / 8-byte load at lane * 16 (+ 8), the 2-wide last group of C4 = 6, 10 one
// 8-byte load at lane * 8.
template <int C4, int C0, int N>
__device__ __forceinline__ void wimg_load(const buf_rsrc wr, const unsigned lane, const unsigned uni, float* dst) {
    if constexpr (N > 0) {
        constexpr int G = C0 / 4, I = C0 - 4 * G, WD = C4 - 4 * G < 4 ? C4 - 4 * G : 4;
        constexpr unsigned GO = (unsigned)(4 * G * 64 + I) * 4u;
        const unsigned lo = lane * (unsigned)(4 * WD);
        if constexpr (I == 0 && WD == 4 && N >= 4) {
            const f32x4 v = buf_load_f32x4(wr, lo, uni + GO);
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
            wimg_load<C4, C0 + 4, N - 4>(wr, lane, uni, dst + 4);
        } else if constexpr (I % 2 == 0 && WD % 2 == 0 && I + 2 <= WD && N >= 2) {
            const f32x2 v = buf_load_f32x2(wr, lo, uni + GO);
            dst[0] = v[0]; dst[1] = v[1];
            wimg_load<C4, C0 + 2, N - 2>(wr, lane, uni, dst + 2);
        } else {
            dst[0] = buf_load_f32(wr, lo, uni + GO);
            wimg_load<C4, C0 + 1, N - 1>(wr, lane, uni, dst + 1);
        }
    }
}
// the image is there: the flag word and the size its writer recorded agree with the plan (wave-uniform: scalar loads)
__device__ __forceinline__ bool wimg_present(const FusedArgs& a) {
    if (!a.wimg) return false;
    const unsigned* h = reinterpret_cast<const unsigned*>(a.wimg);
    return h[0] == kWimgMagic && h[1] == (unsigned)a.wimg_floats;
}

// Timing what-ifs of the static-shape kernel (scripts/build_whatif.py compiles this file with -DTCR_FUSED_WHATIF=<mask> into
// side libraries; WRONG results, never part of the product build): 1 no MFMAs, 2 weights of tap 0 only, 4 LDS operands of tap 0
// only, 8 no barriers, 16 no head, 32 no epilogue stores, 64 no first conv, 512 empty kernel, 1024 no halo-zero passes, 2048 phase stamps
// (scripts/fused_ts.py), 4096 / 8192 the lookahead layers without their weight refills / without LDS operand reads after tap 0,
// 65536 restricts 4096 to conv1_0 (the stride-2 layer 24 -> 32),
// 16384 / 32768 (right results) s_setprio 2 around a tap's MFMA burst / around its operand requests: 110 / 101 us against 98 -- slower, not built in.
#ifndef TCR_FUSED_WHATIF
#define TCR_FUSED_WHATIF 0
#endif
#define TCR_WHATIF(bit) ((TCR_FUSED_WHATIF & (bit)) != 0)
#if TCR_FUSED_WHATIF & (16384 | 32768)
#define TCR_WHATIF_PRIO(bit, level) do { if (TCR_WHATIF(bit)) __builtin_amdgcn_s_setprio(level); } while (0)
#else
#define TCR_WHATIF_PRIO(bit, level) do { } while (0)       // (the host build of tests/emu has no such builtin)
#endif
#if TCR_FUSED_WHATIF & 1
__device__ __forceinline__ f32x4 whatif_nomfma(float a, float b, f32x4 c) { c[0] += a; c[1] += b; return c; }
#define TCR_MFMA(A, B, C) whatif_nomfma((A), (B), (C))
#else
#define TCR_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x4f32((A), (B), (C), 0, 0, 0)
#endif

// NW: wavefronts per workgroup (jobs of a layer are dealt round-robin to them).  R: depth of the weight register ring.
// One layer of the walk for the group's `ng` utterances.  xin: input rows (LDS buffer, or -- first layer -- the feature
// rows in global memory, which then never occupy LDS), in_sz floats per utterance.
template <int NW, int R>
__device__ __forceinline__ void fused_layer(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                            float* lds, const int ng, const int wave, const int r, const int q) {
    const int tpi = L.tin + 2 * kHalo, tpo = L.tout + 2 * kHalo;
    float* yout = lds + a.buf_off[L.out_buf];
    const float* res = L.res_buf >= 0 ? lds + a.buf_off[L.res_buf] : nullptr;
    const int out_sz = L.out_sz;
    const int res_sz = L.res_sz;
    const int npos = ng * L.tout;
    const int ncp = (npos + 31) / 32;               // column pairs (32 positions)
    const int nrt = (L.cout + 15) / 16;             // row tiles (16 output channels)
    const int C4 = L.cin >> 2;
    const int nsteps = L.k * C4;
    const float* w = a.params + L.w_off;
    const float* scale = a.ss + L.ss_off;
    const float* shift = scale + L.c_pad;
    const int wstep = 4 * L.cout;                   // weight floats per K-step (4 input channels of one tap)
    const int xstep = 4 * tpi;                      // LDS floats per K-step within a tap
    // position -> (utterance of the group, frame) without an integer division: (p + 0.5) / tout is never within
    // float round-off of an integer for the p < 2^16 that occur here
    const float inv_tout = 1.0f / (float)L.tout;
    for (int job = wave; job < ncp * nrt; job += NW) {
        const int cp = job / nrt, m = job - cp * nrt;
        // A-fragment element of this lane: W[j][4*c4 + q][16*m + r]; rows beyond Cout are clamped (never stored)
        const int aidx = q * L.cout + min(m * 16 + r, L.cout - 1);
        const int p0 = min(cp * 32 + r, npos - 1), p1 = min(cp * 32 + 16 + r, npos - 1);
        const int g0 = (int)(((float)p0 + 0.5f) * inv_tout), g1 = (int)(((float)p1 + 0.5f) * inv_tout);
        const int t0 = p0 - g0 * L.tout, t1 = p1 - g1 * L.tout;
        const int xo0 = g0 * in_sz + q * tpi + t0 * L.stride + kHalo - L.pad_lo;
        const int xo1 = g1 * in_sz + q * tpi + t1 * L.stride + kHalo - L.pad_lo;
        // folded-BN scale / shift of this lane's 4 output channels: fetched now, consumed after the K loop
        float sc[4], sh[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int co = min(m * 16 + q * 4 + reg, L.cout - 1);
            sc[reg] = scale[co];
            sh[reg] = shift[co];
        }
        f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
        // K-steps s = (tap j, channel quad c4), tap-major.  Weights come from L1/L2 through a 4-deep register
        // ring (uniform base + 32-bit lane offset, clamped instead of branched at the tail); activations are read
        // from the LDS rows at xo + off, where off = c4 * xstep + j is advanced with scalar increments.
        const int last = nsteps - 1;
        float ar[R];
#pragma unroll
        for (int i = 0; i < R; ++i) ar[i] = w[aidx + min(i, last) * wstep];
        // LDS operands are read one step ahead of the MFMAs that consume them (b0/b1 = current step,
        // nb0/nb1 = next step), so the matrix pipe never waits on a ds_read it has just issued.
        int off = xstep, c4 = 1, j = 0;
        if (C4 == 1) { c4 = 0; off = j = 1; }
        float b0 = xin[xo0], b1 = xin[xo1];
#define TCR_FUSED_STEP(AREG, RELOAD)                                                                    \
    {                                                                                                   \
const float nb0 = xin[xo0 + off], nb1 = xin[xo1 + off];     /* (one step past the end: inside the pad) */ \
acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(AREG, b0, acc0, 0, 0, 0);                           \
acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(AREG, b1, acc1, 0, 0, 0);                           \
RELOAD                                                                                          \
b0 = nb0;                                                                                       \
b1 = nb1;                                                                                       \
off += xstep;                                                                                   \
if (++c4 == C4) { c4 = 0; off = ++j; }                                                          \
    }
        int s0 = 0;
        for (; s0 + R <= nsteps; s0 += R) {
#pragma unroll
            for (int i = 0; i < R; ++i) TCR_FUSED_STEP(ar[i], ar[i] = w[aidx + min(s0 + R + i, last) * wstep];)
        }
#pragma unroll
        for (int i = 0; i < R - 1; ++i)
            if (s0 + i < nsteps) TCR_FUSED_STEP(ar[i], )
#undef TCR_FUSED_STEP
        // ---- epilogue, branch-free (round 3, as in fused_layer_s): lanes past the last position / past Cout store into the pad behind
        // the buffers, the residual reads use clamped addresses, the halo zeros come from fused_zero_halo_g ----
        const int dump = a.buf_off[2] + a.group * a.buf_sz[2] + (q * 16 + r) - a.buf_off[L.out_buf];
        const float lo = L.relu ? 0.f : -3.4e38f;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const bool pv = cp * 32 + nt * 16 + r < npos;
            const int g = nt == 0 ? g0 : g1, t = nt == 0 ? t0 : t1;
            const f32x4 ac = nt == 0 ? acc0 : acc1;
            const int base = g * out_sz + kHalo + t;
            float rv[4] = {0.f, 0.f, 0.f, 0.f};
            if (res) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) rv[reg] = res[g * res_sz + min(m * 16 + q * 4 + reg, L.cout - 1) * tpo + kHalo + t];
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int co = m * 16 + q * 4 + reg;
                float v = fmaf(ac[reg], sc[reg], sh[reg]);
                v = res ? fmaxf(v + rv[reg], 0.f) : fmaxf(v, lo);      // tc_resnet.py:40-41
                yout[(pv && co < L.cout) ? base + co * tpo : dump] = v;
            }
        }
    }
}

// The same layer with its shape known at COMPILE time (the flagship configurations: TCResNet8-1.0 at 49 and 98 frames).
// Every K-step of the generic walk above costs ~14 scalar / vector instructions next to its two MFMAs -- step counters, the
// (tap, channel-quad) -> offset bookkeeping, clamped weight indices -- and with 3-8 jobs per barrier phase a wave cannot keep
// the matrix pipe busy at that ratio.  With K, stride, Cin, Cout and T as template parameters the K loop unrolls, the LDS
// operands are read at immediate offsets (c4 * 4 * Tp + tap), the weights at immediate offsets from one per-tap base, and the
// position -> (utterance, frame) split divides by a constant.  Same accumulation order (tap-major, channel quads inner): the
// result is bitwise the generic layer's.
template <int NW, int K, int S, int CIN, int COUT, int TIN>
__device__ __forceinline__ void fused_layer_t(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                              float* lds, const int ng, const int wave, const int r, const int q) {
    constexpr int TOUT = (TIN + S - 1) / S;
    constexpr int PADT = ((TOUT - 1) * S + K - TIN) > 0 ? ((TOUT - 1) * S + K - TIN) : 0;
    constexpr int PADLO = PADT / 2;
    constexpr int TPI = TIN + 2 * kHalo, TPO = TOUT + 2 * kHalo;
    constexpr int C4 = CIN / 4, NRT = (COUT + 15) / 16;
    constexpr int WSTEP = 4 * COUT, XSTEP = 4 * TPI;
    static_assert(CIN % 4 == 0, "channel quads");
    float* yout = lds + a.buf_off[L.out_buf];
    const float* res = L.res_buf >= 0 ? lds + a.buf_off[L.res_buf] : nullptr;
    const int out_sz = L.out_sz;
    const int res_sz = L.res_sz;
    const int npos = ng * TOUT;
    const int ncp = (npos + 31) / 32;
    const float* w = a.params + L.w_off;
    const float* scale = a.ss + L.ss_off;
    const float* shift = scale + L.c_pad;
    for (int job = wave; job < ncp * NRT; job += NW) {
        const int cp = job / NRT, m = job - cp * NRT;
        const int p0 = min(cp * 32 + r, npos - 1), p1 = min(cp * 32 + 16 + r, npos - 1);
        const int g0 = p0 / TOUT, g1 = p1 / TOUT;
        const int t0 = p0 - g0 * TOUT, t1 = p1 - g1 * TOUT;
        const float* wp = w + q * COUT + min(m * 16 + r, COUT - 1);
        const float* x0 = xin + g0 * in_sz + q * TPI + t0 * S + kHalo - PADLO;
        const float* x1 = xin + g1 * in_sz + q * TPI + t1 * S + kHalo - PADLO;
        float sc[4], sh[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int co = min(m * 16 + q * 4 + reg, COUT - 1);
            sc[reg] = scale[co];
            sh[reg] = shift[co];
        }
        f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f}, acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
        // Taps stay a loop (one pointer increment each; unrolling taps AND channel quads lets the scheduler hoist all K * C4 operand
        // loads: 207 VGPRs, half the occupancy).  The weight fragments of a tap live in two half-tap register sets; a set is refilled
        // for the NEXT tap as soon as its MFMAs are issued, so the (L1 / L2) weight loads fly behind the other half's MFMAs instead of
        // in front of the tap (timing what-if: weights fetched once per job would save 12 % of the kernel).
        constexpr int H0 = C4 / 2, H1 = C4 - H0;
        float wa[H0 > 0 ? H0 : 1], wb[H1];
#pragma unroll
        for (int c4 = 0; c4 < H0; ++c4) wa[c4] = wp[c4 * WSTEP];
#pragma unroll
        for (int c4 = 0; c4 < H1; ++c4) wb[c4] = wp[(H0 + c4) * WSTEP];
#pragma unroll 1
        for (int j = 0; j < K; ++j) {
            const int jn = min(j + 1, K - 1);                           // (the last tap refills with itself: branch-free)
            {
                float b0[H0 > 0 ? H0 : 1], b1[H0 > 0 ? H0 : 1];
#pragma unroll
                for (int c4 = 0; c4 < H0; ++c4) { b0[c4] = x0[c4 * XSTEP + j]; b1[c4] = x1[c4 * XSTEP + j]; }
#pragma unroll
                for (int c4 = 0; c4 < H0; ++c4) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[c4], b0[c4], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[c4], b1[c4], acc1, 0, 0, 0);
                }
#pragma unroll
                for (int c4 = 0; c4 < H0; ++c4) wa[c4] = wp[(jn * C4 + c4) * WSTEP];
            }
            {
                float b0[H1], b1[H1];
#pragma unroll
                for (int c4 = 0; c4 < H1; ++c4) { b0[c4] = x0[(H0 + c4) * XSTEP + j]; b1[c4] = x1[(H0 + c4) * XSTEP + j]; }
#pragma unroll
                for (int c4 = 0; c4 < H1; ++c4) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[c4], b0[c4], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[c4], b1[c4], acc1, 0, 0, 0);
                }
#pragma unroll
                for (int c4 = 0; c4 < H1; ++c4) wb[c4] = wp[(jn * C4 + H0 + c4) * WSTEP];
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            if (cp * 32 + nt * 16 + r >= npos) continue;
            const int g = nt == 0 ? g0 : g1, t = nt == 0 ? t0 : t1;
            const f32x4 ac = nt == 0 ? acc0 : acc1;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int co = m * 16 + q * 4 + reg;
                if (co >= COUT) continue;
                float v = fmaf(ac[reg], sc[reg], sh[reg]);
                if (res) v = fmaxf(v + res[g * res_sz + co * TPO + kHalo + t], 0.f);
                else if (L.relu) v = fmaxf(v, 0.f);
                float* dst = yout + g * out_sz + co * TPO + kHalo + t;
                dst[0] = v;
                if (t == 0) { dst[-4] = 0.f; dst[-3] = 0.f; dst[-2] = 0.f; dst[-1] = 0.f; }
                if (t == TOUT - 1) { dst[1] = 0.f; dst[2] = 0.f; dst[3] = 0.f; dst[4] = 0.f; }
            }
        }
    }
}

// Round 3: the static-shape layer with a branch-free epilogue.  The round-2 epilogue above spends ~60 instructions and six exec-mask
// branches per output element (bounds tests, the residual read behind a branch, the halo zeros written by whichever lane owns a row's
// first / last frame).  Here lanes past the group's last position / past Cout store into the pad behind the buffers, the residual
// reads are issued together with clamped addresses, and the halo zeros of the output rows are written by `fused_zero_halo` (one pass
// per layer): 17.5 M instead of 21.3 M VALU and 4.9 M instead of 11 M SALU instructions per launch, bitwise the same results.
// (Tried with it and dropped: the taps fully unrolled into a software pipeline -- weight fragments two / three stages ahead in a
// register ring, LDS operands one stage ahead, a scheduling barrier per stage: 131 / 133 us vs 125 us, SQ_WAIT_INST_ANY UP 11 %.)
// One job of the static-shape layer: NTJ 16-position tiles x 16 output channels (row tile m); cc[nt] = the position index of this lane's
// column in tile nt (>= npos: an empty column -- computed on a clamped address, stored into the pad).
// AHEAD: 0 the rolled tap loop with two half-tap weight sets; 1 a whole tap of weight lookahead.  (Measured and removed, round 6: a ring
// of three full-tap sets running on ACROSS the jobs of a wave -- two taps of lookahead, the next job's first two taps requested behind
// this job's last two: 98.9 us against 95.3 for the one-tap form, 128 registers + 124 B of scratch.)
// TM (time-major plan, kernels.h): cc[nt] is the wave-uniform TILE index (frames 2 c, 2 c + 1 x the 8 utterance slots), `npos` the group's
// utterance count, [jlo, jhi] the job's live taps (fused_tm_taps); OCS: who reads the output rows (0: no convolution -- rows without
// halo; 1 / 2: a stride-1 / stride-2 layer).  A lane's offset inside a tile (its slot and frame half, q * pitch) is the same for every
// tile: the position -> (utterance, frame) division is gone; lanes of an absent frame or utterance read a clamped address and store
// into the pad.
// IMG: weight fragments, scale and shift by 16 / 8-byte loads out of the frozen table's weight image (wimg_load) -- same values, same order.
template <int K, int S, int CIN, int COUT, int TIN, bool HAS_RES, int NTJ, bool WLDS, int AHEAD = 0, bool TM = false, int OCS = 0, bool IMG = false>
__device__ __forceinline__ void fused_job_s(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                            float* yout, const float* res, const float* w, const int npos, const int m, const int (&cc)[NTJ],
                                            const int r, const int q, const int jlo = 0, const int jhi = K - 1, const int wio = 0) {     // wio (IMG): float offset of the layer's fragments in the image
    constexpr int TOUT = (TIN + S - 1) / S;
    constexpr int PADT = ((TOUT - 1) * S + K - TIN) > 0 ? ((TOUT - 1) * S + K - TIN) : 0;
    constexpr int PADLO = PADT / 2;
    // channel pitch of the input / output / shortcut rows and floats per tap: time-major rows are [frame + halo][8]
    constexpr int TPI = TM ? fused_tm_pitch(TIN, true, S) : TIN + 2 * kHalo;
    constexpr int TPO = TM ? fused_tm_pitch(TOUT, OCS != 0, OCS) : TOUT + 2 * kHalo;
    constexpr int TPR = TM ? fused_tm_pitch(TOUT, false, 0) : TPO;
    constexpr int JS = TM ? kTmGroup : 1;
    constexpr int C4 = CIN / 4;
    constexpr int WSTEP = 4 * COUT, XSTEP = 4 * TPI;
    const int out_sz = L.out_sz;
    const int res_sz = L.res_sz;
    const int ja = TM ? jlo : 0, jb = TM ? jhi : K - 1;         // (the other walks: constants)
    int gg[NTJ], tt[NTJ];
    const float* xp[NTJ];
#pragma unroll
    for (int nt = 0; nt < NTJ; ++nt) {
        if constexpr (TM) {
            const int half = (TOUT % 2 == 1 && cc[nt] == TOUT / 2) ? 0 : (r >> 3);
            gg[nt] = half * 8 + min(r & 7, npos - 1);           // this lane's (clamped) place in the tile
            tt[nt] = cc[nt] * 16;
            xp[nt] = xin + q * TPI + (S == 1 ? gg[nt] : 2 * gg[nt] - (gg[nt] & 7)) + tt[nt] * S + kTmGroup * (kHalo - PADLO);
        } else {
        const int p = min(cc[nt], npos - 1);
        gg[nt] = p / TOUT;
        tt[nt] = p - gg[nt] * TOUT;
        xp[nt] = xin + gg[nt] * in_sz + q * TPI + tt[nt] * S + kHalo - PADLO;
        }
    }
    const float* wp = w + q * COUT + min(m * 16 + r, COUT - 1);
    // This lane's four output channels cob .. cob + 3: COUT % 4 == 0, so they are inside Cout or beyond it TOGETHER; a quad beyond it is
    // clamped as a whole (its results go to the pad).  Scale / shift come through ONE buffer descriptor on the table -- a 32-bit lane
    // offset and uniform offsets, eight loads off one address register -- where eight per-lane 64-bit addresses were built per job.
    static_assert(COUT % 4 == 0, "a lane's four output channels are valid or invalid together");
    const int cob = min(m * 16 + q * 4, COUT - 4);
    const buf_rsrc sr = make_rsrc(a.ss);
    const unsigned sl = (unsigned)cob * 4u;
    float sc[4], sh[4];
    if constexpr (IMG) {
        const f32x4 vs = buf_load_f32x4(sr, sl, (unsigned)L.ss_off * 4u), vh = buf_load_f32x4(sr, sl, (unsigned)(L.ss_off + L.c_pad) * 4u);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) { sc[reg] = vs[reg]; sh[reg] = vh[reg]; }
    } else {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        sc[reg] = buf_load_f32(sr, sl, (unsigned)(L.ss_off + reg) * 4u);
        sh[reg] = buf_load_f32(sr, sl, (unsigned)(L.ss_off + L.c_pad + reg) * 4u);
    }
    }
    // (IMG) the image's descriptor, this lane's index and the byte offset of row tile m's first tap; a tap is C4 * 64 floats
    const buf_rsrc ir = make_rsrc(IMG ? a.wimg : a.params);
    const unsigned il = (unsigned)(q * 16 + r);
    const unsigned io = (unsigned)(kWimgHeader + wio + m * (K * C4 * 64)) * 4u;
    constexpr unsigned kTapBytes = (unsigned)(C4 * 64) * 4u;
    f32x4 acc[NTJ];
#pragma unroll
    for (int nt = 0; nt < NTJ; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (AHEAD == 1) {
        // A whole tap of lookahead for the narrow layers (round 6): in the loop below the compiler sinks a half-tap's refill loads to the
        // END of the tap body (ISA: four global_load_dword behind the last MFMA, `s_waitcnt vmcnt(3)` in front of the next tap's first), so
        // with 8 - 12 MFMAs per tap (16 / 24 input channels) every tap waits out an L1 / L2 round trip.  Two full-tap register sets that
        // trade roles (taps unrolled by two: no copies): the NEXT tap's fragments are requested -- through a buffer descriptor: uniform
        // base + constant lane offset + uniform tap offset, no vector address arithmetic -- before this tap's LDS reads and MFMAs.  Same
        // accumulation order: bitwise.
        // (ONE descriptor on the parameter arena for every layer, the layer's offset in the uniform part: a descriptor per layer is four
        //  scalar registers per layer held across the group loop)
        const buf_rsrc wr = make_rsrc(a.params);
        const unsigned wl = (unsigned)(q * COUT + min(m * 16 + r, COUT - 1)) * 4u;
        const unsigned wo = (unsigned)L.w_off * 4u;
        float w0[C4], w1[C4];
        if constexpr (IMG) wimg_load<C4, 0, C4>(ir, il, io + (unsigned)ja * kTapBytes, w0);
        else {
#pragma unroll
        for (int c4 = 0; c4 < C4; ++c4) w0[c4] = buf_load_f32(wr, wl, wo + (unsigned)((ja * C4 + c4) * WSTEP) * 4u);
        }
        auto tap = [&](const int j, const float (&wu)[C4], float (&wf)[C4], const bool fill) {
            TCR_WHATIF_PRIO(32768, 2);
            if (fill && !(TCR_WHATIF(4096) && (!TCR_WHATIF(65536) || (S == 2 && CIN == 24 && COUT == 32)))) {
                if constexpr (IMG) wimg_load<C4, 0, C4>(ir, il, io + (unsigned)(j + 1) * kTapBytes, wf);
                else {
#pragma unroll
                for (int c4 = 0; c4 < C4; ++c4) wf[c4] = buf_load_f32(wr, wl, wo + (unsigned)(((j + 1) * C4 + c4) * WSTEP) * 4u);
                }
            }
            float b[NTJ][C4];
            if (TCR_WHATIF(8192) && j > 0) {
#pragma unroll
                for (int c4 = 0; c4 < C4; ++c4)
#pragma unroll
                    for (int nt = 0; nt < NTJ; ++nt) b[nt][c4] = wu[c4] + (float)nt;       // (timing what-if: no LDS operand reads after tap 0)
            } else {
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4)
#pragma unroll
                for (int nt = 0; nt < NTJ; ++nt) b[nt][c4] = xp[nt][c4 * XSTEP + JS * j];
            }
            __builtin_amdgcn_sched_barrier(0);                  // (the requests stay in front of the tap's MFMAs)
            TCR_WHATIF_PRIO(16384, 2);
            TCR_WHATIF_PRIO(32768, 0);
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4)
#pragma unroll
                for (int nt = 0; nt < NTJ; ++nt) acc[nt] = TCR_MFMA(wu[c4], b[nt][c4], acc[nt]);
            TCR_WHATIF_PRIO(16384, 0);
        };
        if constexpr (TM) {
            // the live taps only: 5 - 9 of them, an odd or an even count
            int j = ja;
#pragma unroll 1
            for (; j + 2 <= jb; j += 2) {
                tap(j, w0, w1, true);
                tap(j + 1, w1, w0, true);
            }
            if (j == jb) {
                tap(j, w0, w1, false);
            } else {
                tap(j, w0, w1, true);
                tap(j + 1, w1, w0, false);
            }
        } else {
#pragma unroll 1
        for (int j = 0; j + 2 < K; j += 2) {
            tap(j, w0, w1, true);
            tap(j + 1, w1, w0, true);
        }
        if constexpr (K % 2 == 1) {
            tap(K - 1, w0, w1, false);
        } else {
            tap(K - 2, w0, w1, true);
            tap(K - 1, w1, w0, false);
        }
        }
    } else {
    // rolled taps, two half-tap weight sets refilled for the next tap (the round-2 loop).  Weights in global memory (`w` is
    // a.params + L.w_off) are read through the buffer descriptor as in the lookahead form (constant lane offset + the tap's uniform
    // offset: no 64-bit vector address per load); the small-batch kernel's weights are in LDS.
    constexpr int H0 = C4 / 2, H1 = C4 - H0;
    const buf_rsrc wr = make_rsrc(a.params);
    const unsigned wl = (unsigned)(q * COUT + min(m * 16 + r, COUT - 1)) * 4u;
    const unsigned wo = (unsigned)L.w_off * 4u;
    auto wld = [&](const int step) {
        if constexpr (WLDS) return wp[step * WSTEP];
        else return buf_load_f32(wr, wl, wo + (unsigned)(step * WSTEP) * 4u);
    };
    float wa[H0 > 0 ? H0 : 1], wb[H1];
    // a half-tap set of tap j (IMG: its aligned runs of 4 / 2 channel quads, one load each)
    auto wfill_a = [&](const int j) {
        if constexpr (IMG) wimg_load<C4, 0, H0>(ir, il, io + (unsigned)j * kTapBytes, wa);
        else {
#pragma unroll
            for (int c4 = 0; c4 < H0; ++c4) wa[c4] = wld(j * C4 + c4);
        }
    };
    auto wfill_b = [&](const int j) {
        if constexpr (IMG) wimg_load<C4, H0, H1>(ir, il, io + (unsigned)j * kTapBytes, wb);
        else {
#pragma unroll
            for (int c4 = 0; c4 < H1; ++c4) wb[c4] = wld(j * C4 + H0 + c4);
        }
    };
    wfill_a(ja);
    wfill_b(ja);
    // (throughput kernels: rolled taps -- 128-register budget; small-batch kernel: unrolled, the LDS operand and weight reads of the
    //  following taps move ahead of the MFMAs)
    constexpr int kTapUnroll = WLDS ? K : 1;
#pragma unroll kTapUnroll
    for (int j = ja; j <= jb; ++j) {
        const int jn = TCR_WHATIF(2) ? 0 : min(j + 1, jb);
        const int jx = TCR_WHATIF(4) ? 0 : JS * j;
        {
            float b[NTJ][H0 > 0 ? H0 : 1];
#pragma unroll
            for (int c4 = 0; c4 < H0; ++c4)
#pragma unroll
                for (int nt = 0; nt < NTJ; ++nt) b[nt][c4] = xp[nt][c4 * XSTEP + jx];
#pragma unroll
            for (int c4 = 0; c4 < H0; ++c4)
#pragma unroll
                for (int nt = 0; nt < NTJ; ++nt) acc[nt] = TCR_MFMA(wa[c4], b[nt][c4], acc[nt]);
            wfill_a(jn);
        }
        {
            float b[NTJ][H1];
#pragma unroll
            for (int c4 = 0; c4 < H1; ++c4)
#pragma unroll
                for (int nt = 0; nt < NTJ; ++nt) b[nt][c4] = xp[nt][(H0 + c4) * XSTEP + jx];
#pragma unroll
            for (int c4 = 0; c4 < H1; ++c4)
#pragma unroll
                for (int nt = 0; nt < NTJ; ++nt) acc[nt] = TCR_MFMA(wb[c4], b[nt][c4], acc[nt]);
            wfill_b(jn);
        }
    }
    }
    // ---- epilogue: folded BN (+ shortcut) (+ ReLU) -> LDS rows ----
    // One address per tile and a channel pitch that is 0 in the lanes that store into the pad (the pad holds one float per lane): the four
    // stores of a tile walk one pointer by that pitch, one add each, where every store chose between its row and the pad behind an exec-mask branch.
    const int dump = a.buf_off[2] + a.group * a.buf_sz[2] + (q * 16 + r) - a.buf_off[L.out_buf];
    const float lo = L.relu ? 0.f : -3.4e38f;
    const bool cv = COUT % 16 == 0 || m * 16 + q * 4 < COUT;
    float rv[NTJ][4];
    if (HAS_RES) {
#pragma unroll
        for (int nt = 0; nt < NTJ; ++nt) {
            const int rb = TM ? cob * TPR + tt[nt] + gg[nt] : gg[nt] * res_sz + cob * TPO + kHalo + tt[nt];       // (clamped position, clamped quad: inside the rows)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) rv[nt][reg] = res[rb + reg * TPR];
        }
    }
#pragma unroll
    for (int nt = 0; nt < NTJ; ++nt) {
        const bool ok = (TM ? 2 * cc[nt] + (r >> 3) < TOUT && (r & 7) < npos : cc[nt] < npos) && cv && !TCR_WHATIF(32);
        const f32x4 ac = acc[nt];
        float* po = yout + (ok ? (TM ? tt[nt] + r + (OCS != 0 ? kTmGroup * kHalo : 0) : gg[nt] * out_sz + kHalo + tt[nt]) + cob * TPO : dump);
        const int pitch = ok ? TPO : 0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float v = fmaf(ac[reg], sc[reg], sh[reg]);
            if (HAS_RES) v = fmaxf(v + rv[nt][reg], 0.f);       // tc_resnet.py:40-41
            else v = fmaxf(v, lo);
            *po = v;
            po += pitch;
        }
    }
}

template <int NW, int K, int S, int CIN, int COUT, int TIN, bool HAS_RES, int NTJ = 2, bool WLDS = false>
__device__ __forceinline__ void fused_layer_s(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                              float* lds, const int ng, const int wave, const int r_in, const int q_in,
                                              const int w_lds = 0) {     // WLDS: this layer's weights are staged in LDS at float offset w_lds (small-batch kernel)
    // lane geometry re-derived from an opaque zero: the per-lane address arithmetic of ten layers must not be hoisted out of the group
    // loop, where it would stay live through every other layer (the kernel runs at a 128-register budget)
    const int oz = opaque_zero();
    const int r = r_in + oz, q = q_in + oz;
    constexpr int TOUT = (TIN + S - 1) / S;
    constexpr int NRT = (COUT + 15) / 16;
    constexpr int JP = 16 * NTJ;            // positions per job
    static_assert(CIN % 4 == 0, "channel quads");
    static_assert(NTJ == 1 || NTJ == 2 || NTJ == 4, "one, two or four 16-position tiles per job");
    float* yout = lds + a.buf_off[L.out_buf];
    const float* res = L.res_buf >= 0 ? lds + a.buf_off[L.res_buf] : nullptr;
    const int npos = ng * TOUT;
    const int ncp = (npos + JP - 1) / JP;
    const float* w = WLDS ? lds + w_lds : a.params + L.w_off;
    // Which of a job's positions a lane's tile columns hold (the columns of the implicit GEMM are independent: any assignment
    // gives the same sums).  One ds_read_b32 serves lanes (q, q + 1) x 16 columns against 32 banks: with stride 2 consecutive columns
    // are 2 floats apart and the odd row pitch puts row q + 1 on the other bank parity; with stride 1 the columns of a tile are every
    // OTHER position (tile 0 the even, tile 1 the odd ones of a run of 32) for the same picture.  The host pads the per-utterance stride so that the
    // pattern continues across the utterances of a group (net.cpp: fused_strides).  PMC, TCResNet8 at 49 frames: see OPTLOG.md.
    // NTJ = 4 (round 5 experiment; the 16 / 24-channel layers at 25 frames): a weight fragment feeds four MFMAs instead of two -- those layers have
    // 4 - 6 channel quads, i.e. 8 - 12 MFMAs between two dependent weight loads of a tap, and 14 jobs for 8 waves; with 64-position jobs a tap's
    // loads sit behind 16 - 24 MFMAs and a layer is one round of <= 8 jobs.  Same sums (columns are independent), bitwise -- and no faster
    // (phase stamps, scripts/fused_ts.py: block 0's first phase 37.5 -> 31.8 k cycles, its second 39.5 -> 43.4 k: the two workgroups of a CU
    // share the matrix pipes, a shorter phase of one lengthens the other's).
    constexpr bool IL = S == 1;
    for (int job = wave; job < ncp * NRT; job += NW) {
        const int cp = job / NRT, m = job - cp * NRT;
        int cc[NTJ];
#pragma unroll
        for (int nt = 0; nt < NTJ; ++nt) cc[nt] = (IL && NTJ > 1) ? cp * JP + 32 * (nt >> 1) + 2 * r + (nt & 1) : cp * JP + 16 * nt + r;
        fused_job_s<K, S, CIN, COUT, TIN, HAS_RES, NTJ, WLDS>(a, L, xin, in_sz, yout, res, w, npos, m, cc, r, q);
    }
}

// Zero halos of time-major rows [COUT][(TOUT + 8) x 8 | pad to PITCH]: two contiguous runs of 32 floats per channel, 16 bytes per thread.
template <int NT, int COUT, int TOUT, int PITCH>
__device__ __forceinline__ void fused_zero_halo_tm(float* yout, const int tid_in) {
    if (TCR_WHATIF(1024)) return;
    const int tid = tid_in + opaque_zero();
    for (int i = tid; i < COUT * 16; i += NT) {
        float4* p = reinterpret_cast<float4*>(yout + (i >> 4) * PITCH + ((i & 8) ? kTmGroup * (kHalo + TOUT) : 0) + 4 * (i & 7));
        *p = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// A layer of the time-major plan (kernels.h: fused_tm_pitch / fused_tm_taps / fused_tm_deal): groups of 8 utterances, positions ordered
// p = 8 * frame + utterance, so a 16-position tile is two frames of every utterance and a tap whose input frame lies in the SAME-padding
// halo for both frames is dead for the whole tile -- wave-uniformly, and known at compile time.  Such taps multiplied finite weights
// with zeros into accumulators that start at +0; here their MFMAs, operand reads and weight fetches are not issued (fused_job_s walks the
// job's live taps [lo, hi] in the same order: bitwise).  The waves' jobs come from the compile-time deal, read with scalar loads.
template <int NW, int K, int S, int CIN, int COUT, int TIN, bool HAS_RES, int OCS, int AHEAD, bool IMG = false>
__device__ __forceinline__ void fused_layer_tm(const FusedArgs& a, const FusedLayer& L, float* lds, const int ng, const int wave, const int r_in, const int q_in, const int wio = 0) {
    constexpr int TOUT = (TIN + S - 1) / S;
    constexpr int PADT = ((TOUT - 1) * S + K - TIN) > 0 ? ((TOUT - 1) * S + K - TIN) : 0;
    static constexpr FusedTmDeal deal = fused_tm_deal(K, S, CIN, COUT, TIN, PADT / 2, NW);
    static_assert(fused_tm_deal_fits(deal, NW), "a wave's jobs exceed the deal's table (kTmMaxJobs)");
    float* yout = lds + a.buf_off[L.out_buf];
    if constexpr (OCS != 0) fused_zero_halo_tm<NW * 64, COUT, TOUT, fused_tm_pitch(TOUT, true, OCS)>(yout, (int)threadIdx.x);
    const int oz = opaque_zero();
    const int r = r_in + oz, q = q_in + oz;
    const float* xin = lds + a.buf_off[L.in_buf];
    const float* res = L.res_buf >= 0 ? lds + a.buf_off[L.res_buf] : nullptr;
    const float* w = a.params + L.w_off;
    const int n = deal.n[wave];
    for (int i = 0; i < n; ++i) {
        const unsigned jw = deal.job[wave][i];
        const int m = (int)(jw & 15u), c = (int)(jw >> 4 & 63u), lo = (int)(jw >> 11 & 15u), hi = (int)(jw >> 15 & 15u);
        if (jw >> 10 & 1u) {
            const int cc[2] = {c, c + 1};
            fused_job_s<K, S, CIN, COUT, TIN, HAS_RES, 2, false, AHEAD, true, OCS, IMG>(a, L, xin, 0, yout, res, w, ng, m, cc, r, q, lo, hi, wio);
        } else {
            const int cc[1] = {c};
            fused_job_s<K, S, CIN, COUT, TIN, HAS_RES, 1, false, AHEAD, true, OCS, IMG>(a, L, xin, 0, yout, res, w, ng, m, cc, r, q, lo, hi, wio);
        }
    }
}

// The same layer with its work dealt in UNITS of one 16-position tile x 16 output channels (round 6).  fused_layer_s deals whole jobs of
// two tiles round-robin: 14 jobs on 8 waves in block 0 (a SIMD hosts waves w and w + 4 of the workgroup: 4 / 4 / 3 / 3 jobs), 6 jobs in
// block 2 (2 / 2 / 1 / 1: two SIMDs carry twice the matrix work of the other two), and the positions of a group are padded to 32.  Here a
// wave owns a contiguous run of units, as even as units allow -- the first U mod 8 waves one more, so the SIMDs differ by at most one unit
// (block 0: 7 / 7 / 6 / 6 of 26 units instead of 8 / 8 / 6 / 6 of 28; block 1: 14 units instead of 16; block 2: 3 / 3 / 3 / 3 instead of
// 4 / 4 / 2 / 2) --, and walks it two units at a time where both lie in the same row tile (one weight fragment feeds both), one otherwise.
// Columns of the implicit GEMM are independent: bitwise the job form.  Stride-1 layers keep "a tile = every other position of a run of
// 32" (the bank picture above); a last run of <= 16 positions is one tile of consecutive positions.
template <int NW, int K, int S, int CIN, int COUT, int TIN, bool HAS_RES, int AHEAD = 0>
__device__ __forceinline__ void fused_layer_u(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                              float* lds, const int ng, const int wave, const int r_in, const int q_in) {
    const int oz = opaque_zero();
    const int r = r_in + oz, q = q_in + oz;
    constexpr int TOUT = (TIN + S - 1) / S;
    constexpr int NRT = (COUT + 15) / 16;
    constexpr bool IL = S == 1;
    float* yout = lds + a.buf_off[L.out_buf];
    const float* res = L.res_buf >= 0 ? lds + a.buf_off[L.res_buf] : nullptr;
    const int npos = ng * TOUT;
    const int full = npos >> 5, rem = npos & 31;
    const int nt16 = IL ? 2 * full + (rem == 0 ? 0 : (rem <= 16 ? 1 : 2)) : (npos + 15) >> 4;
    const int il_end = (IL && rem > 0 && rem <= 16) ? 2 * full : nt16;          // tiles from il_end on: consecutive positions
    const int U = NRT * nt16;
    const int per = U / NW, extra = U - per * NW;
    // (measured and removed: the two workgroups of a CU handing their spare units to different SIMDs -- waves rotated by two in every
    //  other workgroup, by blockIdx bit 8 or bit 3: 96.5 / 95.9 us against 95.9; SIMD mates -- waves w and w + 4 -- walking an odd run single
    //  unit first so that their prologues / epilogues do not coincide, also flipped per 256 workgroups: 97.4 / 96.8 against 96.3 - 97.6)
    int u = wave * per + min(wave, extra);
    const int end = u + per + (wave < extra ? 1 : 0);
    const float* w = a.params + L.w_off;
    auto col = [&](int c) { return (IL && c < il_end) ? (c >> 1) * 32 + 2 * r + (c & 1) : (IL ? full * 32 + r : c * 16 + r); };
    while (u < end) {
        const int m = u / nt16, c = u - m * nt16;
        if (c + 1 < nt16 && u + 1 < end) {
            const int cc[2] = {col(c), col(c + 1)};
            fused_job_s<K, S, CIN, COUT, TIN, HAS_RES, 2, false, AHEAD>(a, L, xin, in_sz, yout, res, w, npos, m, cc, r, q);
            u += 2;
        } else {
            const int cc[1] = {col(c)};
            fused_job_s<K, S, CIN, COUT, TIN, HAS_RES, 1, false, AHEAD>(a, L, xin, in_sz, yout, res, w, npos, m, cc, r, q);
            u += 1;
        }
    }
}

// Resident weights for a nine-tap layer of <= 24 input channels (TCResNet8's conv0_1, 24 -> 24).  In fused_layer_u a wave walks its 3 - 4
// units as ~2 jobs and every job's nine taps each start with weight loads from L2 that the tap's MFMAs wait for: ~18 dependent round trips
// per wave and phase.  All units of a wave that lie in one 16-channel row tile use the SAME K x CIN / 4 fragments (54 registers), so here
// the wave requests that set ONCE -- in front of the barrier that precedes the phase, where it holds no job state (fused_resident_request)
// -- and walks a run of units dealt inside one row tile (fused_deal_run, kernels.h) out of those registers; only the LDS operands (one
// tap ahead) are read per unit.  Per output tile the MFMA sequence is the one of fused_job_s (taps outer, channel quads inner, same
// fragments): bitwise.  The barrier in front of the phase is __syncthreads(), whose fence waits for the request (vmcnt(0)): one round
// trip per phase, shared with the wait for the slowest wave.  Phase stamps (OPTLOG "Resident weights"): conv0_1 35.6 -> 29.6 k cycles per
// group, what the phase takes with its weight refills removed (28.2 k); requested BEHIND the barrier the gain is gone (35.3 k).  conv0_0
// (16 -> 24) in this form gains nothing (as its no-refill what-if said) and its request lengthens the first conv's phase: not used there.
template <int NW, int K, int CIN, int COUT, bool IMG = false>
__device__ __forceinline__ void fused_resident_request(const FusedArgs& a, const FusedLayer& L, const int wave, const int r_in, const int q_in,
                                                       float (&ws)[K * (CIN / 4)], const int wio = 0) {
    constexpr int NRT = (COUT + 15) / 16, C4 = CIN / 4, WSTEP = 4 * COUT;
    static_assert(NW % NRT == 0, "the waves split evenly over the row tiles");
    const int oz = opaque_zero();          // (keeps the request inside the group loop: hoisted, the set would live through every layer)
    const int r = r_in + oz, q = q_in + oz;
    const int m = wave / (NW / NRT);       // this wave's row tile (fused_deal_run); requested whether or not its run is empty
    if constexpr (IMG) {            // (the image's row tile m: K taps of C4 * 64 floats, wimg_load)
        const buf_rsrc ir = make_rsrc(a.wimg);
        const unsigned io = (unsigned)(kWimgHeader + wio + m * (K * C4 * 64)) * 4u;
#pragma unroll
        for (int j = 0; j < K; ++j) wimg_load<C4, 0, C4>(ir, (unsigned)(q * 16 + r), io + (unsigned)(j * C4 * 64) * 4u, ws + j * C4);
    } else {
    const buf_rsrc wr = make_rsrc(a.params + L.w_off);
    const unsigned wl = (unsigned)(q * COUT + min(m * 16 + r, COUT - 1)) * 4u;
#pragma unroll
    for (int i = 0; i < K * C4; ++i) ws[i] = buf_load_f32(wr, wl, (unsigned)(i * WSTEP) * 4u);      // i = tap * C4 + channel quad
    }
}

template <int NW, int K, int S, int CIN, int COUT, int TIN, bool HAS_RES, bool TM = false, int OCS = 0, bool IMG = false>
__device__ __forceinline__ void fused_layer_r(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                              float* lds, const int ng, const int wave, const int r_in, const int q_in,
                                              const float (&ws)[K * (CIN / 4)]) {
    const int oz = opaque_zero();
    const int r = r_in + oz, q = q_in + oz;
    constexpr int TOUT = (TIN + S - 1) / S;
    constexpr int NRT = (COUT + 15) / 16;
    constexpr bool IL = S == 1;
    constexpr int PADT = ((TOUT - 1) * S + K - TIN) > 0 ? ((TOUT - 1) * S + K - TIN) : 0;
    constexpr int PADLO = PADT / 2;
    // (time-major plan: pitches per channel, 8 floats per tap, tiles of two frames -- as fused_job_s; the walk stays whole: see OPTLOG)
    constexpr int TPI = TM ? fused_tm_pitch(TIN, true, S) : TIN + 2 * kHalo;
    constexpr int TPO = TM ? fused_tm_pitch(TOUT, OCS != 0, OCS) : TOUT + 2 * kHalo;
    constexpr int TPR = TM ? fused_tm_pitch(TOUT, false, 0) : TPO;
    constexpr int JS = TM ? kTmGroup : 1;
    constexpr int C4 = CIN / 4, XSTEP = 4 * TPI;
    float* yout = lds + a.buf_off[L.out_buf];
    const float* res = L.res_buf >= 0 ? lds + a.buf_off[L.res_buf] : nullptr;
    const int out_sz = L.out_sz;
    const int res_sz = L.res_sz;
    const int npos = TM ? kTmGroup * TOUT : ng * TOUT;
    const int full = npos >> 5, rem = npos & 31;
    const int nt16 = TM ? (TOUT + 1) / 2 : IL ? 2 * full + (rem == 0 ? 0 : (rem <= 16 ? 1 : 2)) : (npos + 15) >> 4;          // (tiles and columns: as fused_layer_u)
    const int il_end = (IL && rem > 0 && rem <= 16) ? 2 * full : nt16;
    const FusedRun run = fused_deal_run(NRT, nt16, NW, wave);
    const int m = run.m;
    static_assert(COUT % 4 == 0, "a lane's four output channels are valid or invalid together");
    const buf_rsrc sr = make_rsrc(a.ss);                        // (scale / shift of the lane's channel quad: as fused_job_s)
    const unsigned sl = (unsigned)min(m * 16 + q * 4, COUT - 4) * 4u;
    float sc[4], sh[4];
    if constexpr (IMG) {
        const f32x4 vs = buf_load_f32x4(sr, sl, (unsigned)L.ss_off * 4u), vh = buf_load_f32x4(sr, sl, (unsigned)(L.ss_off + L.c_pad) * 4u);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) { sc[reg] = vs[reg]; sh[reg] = vh[reg]; }
    } else {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        sc[reg] = buf_load_f32(sr, sl, (unsigned)(L.ss_off + reg) * 4u);
        sh[reg] = buf_load_f32(sr, sl, (unsigned)(L.ss_off + L.c_pad + reg) * 4u);
    }
    }
    // this lane's position in column tile c -> (utterance of the group, frame); computed twice per unit, in front of the taps for the operand
    // address and again behind them for the stores, so that nothing but the address is live across the 9 x C4 MFMAs (the 128-register budget)
    auto place = [&](const int c, const int rr, int& g, int& t) {
        if constexpr (TM) {         // g: this lane's (clamped) place in the tile, t: the tile's first float
            g = ((TOUT % 2 == 1 && c == TOUT / 2) ? 0 : (rr >> 3)) * 8 + min(rr & 7, ng - 1);
            t = 16 * c;
            return 2 * c + (rr >> 3) < TOUT && (rr & 7) < ng;
        }
        const int cc = (IL && c < il_end) ? (c >> 1) * 32 + 2 * rr + (c & 1) : (IL ? full * 32 + rr : c * 16 + rr);
        const int p = min(cc, npos - 1);
        g = p / TOUT;
        t = p - g * TOUT;
        return cc < npos;
    };
    for (int c = run.c0; c < run.c1; ++c) {
        int g, t;
        place(c, r, g, t);
        const float* xp = TM ? xin + q * TPI + (S == 1 ? g : 2 * g - (g & 7)) + t * S + kTmGroup * (kHalo - PADLO)
                             : xin + g * in_sz + q * TPI + t * S + kHalo - PADLO;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        // LDS operands: one register per channel quad, refilled for the next tap as soon as its MFMA has issued (a tap = C4 MFMAs of lookahead)
        // (time-major, measured and removed: the tile's dead taps skipped behind a wave-uniform test per tap of this unrolled walk --
        //  74.5 - 75.3 us against 74.6 - 74.7 with the walk whole: the four edge tiles of 13 save 120 of 1404 MFMAs and pay nine scalar branches per unit)
        float b[C4];
#pragma unroll
        for (int c4 = 0; c4 < C4; ++c4) b[c4] = xp[c4 * XSTEP];
#pragma unroll
        for (int j = 0; j < K; ++j) {
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4) {
                acc = TCR_MFMA(ws[j * C4 + c4], b[c4], acc);
                if (j + 1 < K) b[c4] = xp[c4 * XSTEP + (TCR_WHATIF(4) ? 0 : JS * (j + 1))];
            }
        }
        // ---- epilogue: folded BN (+ shortcut) (+ ReLU) -> LDS rows (as fused_job_s) ----
        const int oe = opaque_zero_after(acc[0]);
        const int re = r_in + oe, qe = q_in + oe;
        const bool pv = place(c, re, g, t);
        const int dump = a.buf_off[2] + a.group * a.buf_sz[2] + (qe * 16 + re) - a.buf_off[L.out_buf];
        const float lo = L.relu ? 0.f : -3.4e38f;
        const int cob = min(m * 16 + qe * 4, COUT - 4);
        float rv[4];
        if (HAS_RES) {
            const int rb = TM ? cob * TPR + t + g : g * res_sz + cob * TPO + kHalo + t;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) rv[reg] = res[rb + reg * TPR];
        }
        const bool ok = pv && (COUT % 16 == 0 || m * 16 + qe * 4 < COUT) && !TCR_WHATIF(32);
        float* po = yout + (ok ? (TM ? t + re + (OCS != 0 ? kTmGroup * kHalo : 0) : g * out_sz + kHalo + t) + cob * TPO : dump);
        const int pitch = ok ? TPO : 0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            float v = fmaf(acc[reg], sc[reg], sh[reg]);
            if (HAS_RES) v = fmaxf(v + rv[reg], 0.f);       // tc_resnet.py:40-41
            else v = fmaxf(v, lo);
            *po = v;
            po += pitch;
        }
    }
}

// First conv of the static-shape kernel (3 x 1, 40 -> 16, stride 1), activations straight from global memory.  In the generic form
// every K-step's two operand loads were issued ONE MFMA ahead of their use (ISA: `s_waitcnt vmcnt(1)` in front of each MFMA): 30
// exposed L1 / L2 / HBM latencies per job -- the layer took 25 us of the kernel's 125 (timing what-if, scripts/whatif_net.py) for
// 10 % of its MFMAs.  Here a job requests ALL its operands up front (per lane 10 channel quads x 3 taps = three consecutive
// floats each, and the 30 weight fragments; a job is 16 positions so that this fits the register budget), then runs its 30 MFMAs:
// one exposed latency per job.  Same accumulation order.  (Measured and removed, round 6: the next job's activations requested a whole job
// ahead -- 90 operand registers, 128 + 200 B of scratch: 103.7 us against 95.4 -- and half a job ahead in two sets of 15 -- less scratch
// than this form, 96.4 against 95.3: the phase reads the whole feature tensor, 37 MB at batch 4096, with every wave of the chip asking at
// the same moment; it is not a per-job latency.)
// TM (time-major plan): the rows it writes are [channel][frame + halo][8].  1: the jobs stay 16 consecutive frames of an utterance -- a lane
// row's global reads stay one 64-byte run per channel and tap, its LDS stores are 8 floats apart (4-way bank conflicts on four stores per
// job); 2: a job is two frames of every utterance -- conflict-free stores, the reads of a lane row split over 8 utterances (see OPTLOG
// for the measurement that chose).
#ifndef TCR_TM_CONV0
#define TCR_TM_CONV0 1
#endif
template <int NW, int T0, bool WLDS = false, int TM = 0, bool IMG = false>
__device__ __forceinline__ void fused_conv0_s(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                              float* lds, const int ng, const int wave, const int r_in, const int q_in,
                                              const int w_lds = 0, const int wio = 0) {
    const int oz = opaque_zero();
    const int r = r_in + oz, q = q_in + oz;
    constexpr int K = 3, CIN = 40, COUT = 16, C4 = CIN / 4;
    constexpr int TPI = T0 + 2 * kHalo, TPO = TM ? fused_tm_pitch(T0, true, 2) : TPI, TOUT = T0, PADLO = 1;
    constexpr int WSTEP = 4 * COUT, XSTEP = 4 * TPI;
    float* yout = lds + a.buf_off[L.out_buf];
    const int out_sz = L.out_sz;
    const int npos = ng * TOUT;
    const int nct = TM == 2 ? (TOUT + 1) / 2 : (npos + 15) / 16;
    const float* w = WLDS ? lds + w_lds : a.params + L.w_off;
    const float* scale = a.ss + L.ss_off;
    const float* shift = scale + L.c_pad;
    for (int job = wave; job < nct; job += NW) {            // job = 16 positions x 16 channels (30 + 30 operand registers)
        const int p0 = min(job * 16 + r, npos - 1);
        const int g0 = TM == 2 ? min(r & 7, ng - 1) : p0 / TOUT;
        const int t0 = TM == 2 ? min(2 * job + (r >> 3), TOUT - 1) : p0 - g0 * TOUT;
        const float* wp = w + q * COUT + r;
        const float* x0 = xin + g0 * in_sz + q * TPI + t0 + kHalo - PADLO;
        float b0[C4][K], wf[K][C4];
#pragma unroll
        for (int c4 = 0; c4 < C4; ++c4)
#pragma unroll
            for (int j = 0; j < K; ++j) b0[c4][j] = x0[c4 * XSTEP + j];
        float sc[4], sh[4];
        if constexpr (IMG && !WLDS) {       // (one row tile: the image's taps follow one another, wimg_load; scale / shift of the lane's channel quad)
            const buf_rsrc ir = make_rsrc(a.wimg), sr = make_rsrc(a.ss);
#pragma unroll
            for (int j = 0; j < K; ++j) wimg_load<C4, 0, C4>(ir, (unsigned)(q * 16 + r), (unsigned)(kWimgHeader + wio + j * C4 * 64) * 4u, wf[j]);
            const f32x4 vs = buf_load_f32x4(sr, (unsigned)q * 16u, (unsigned)L.ss_off * 4u), vh = buf_load_f32x4(sr, (unsigned)q * 16u, (unsigned)(L.ss_off + L.c_pad) * 4u);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) { sc[reg] = vs[reg]; sh[reg] = vh[reg]; }
        } else {
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4) wf[j][c4] = wp[(j * C4 + c4) * WSTEP];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            sc[reg] = scale[q * 4 + reg];
            sh[reg] = shift[q * 4 + reg];
        }
        }
        f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f};
        TCR_WHATIF_PRIO(16384, 2);
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4) acc0 = TCR_MFMA(wf[j][c4], b0[c4][j], acc0);
        TCR_WHATIF_PRIO(16384, 0);
        const int dump = a.buf_off[2] + a.group * a.buf_sz[2] + (q * 16 + r) - a.buf_off[L.out_buf];
        const float lo = L.relu ? 0.f : -3.4e38f;
        const bool pv = TM == 2 ? 2 * job + (r >> 3) < TOUT && (r & 7) < ng : job * 16 + r < npos;
        const int base = TM ? (kHalo + t0) * kTmGroup + g0 : g0 * out_sz + kHalo + t0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const float v = fmaxf(fmaf(acc0[reg], sc[reg], sh[reg]), lo);
            yout[pv ? base + (q * 4 + reg) * TPO : dump] = v;
        }
    }
}

// Head of the static-shape kernel: avg-pool by all threads, then ONE wave runs fc / fc2 on the matrix cores (D[output][utterance], the
// arrangement of head.hip: bitwise the fmaf chain of `fused_head`), the softmax in registers with the class sum carried through the
// three 16-lane rows in class order (bitwise the sequential sum of `fused_head`), and the stores.  `fused_head` -- runtime shapes,
// 48 dependent global weight loads per dot product in batches of 8, twelve expf per thread -- cost 20 us of the kernel's 125.
// TM (time-major plan): the block output's rows are [channel][frame][8], no halo -- a frame's 8 utterances are neighbours, pooled with stride 8.
template <int NT, int FC, int FT, int NCLS, bool TM = false>
__device__ __forceinline__ void fused_head_s(const FusedArgs& a, float* lds, const int n0, const int ng, const int tid) {
    static_assert(FC % 4 == 0 && NCLS + 2 <= 16, "one 16-row MFMA tile holds the logits and the two range outputs");
    constexpr int TP = TM ? fused_tm_pitch(FT, false, 0) : FT + 2 * kHalo;
    constexpr int TS = TM ? kTmGroup : 1;
    const float* fb = lds + a.buf_off[a.feat_buf];
    const int fsz = a.feat_sz;
    float* pooled = lds + a.buf_off[(a.feat_buf + 1) % 3];
    const int lane = tid & 63, r = lane & 15, q = lane >> 4;
    // wave 0: the weight fragments are requested before the pooling phase (their latency hides behind it)
    float af[FC / 4];
    if (tid < 64) {
        // (the lane geometry behind an opaque zero keeps these loads AND their twelve 64-bit lane addresses inside the group loop: hoisted, the
        //  addresses lived through every layer -- they were 96 of the kernel's 116 B of scratch per lane, stored at entry, reloaded here)
        const int zero = opaque_zero();
        const int rz = r + zero, qz = q + zero;
#pragma unroll
        for (int s = 0; s < FC / 4; ++s) {
            const int c = 4 * s + qz;
            const float* src = rz < NCLS ? a.params + a.fc_off + c * NCLS + rz : a.params + a.fc2_off + c * 2 + min(rz - NCLS, 1);
            const float v = src[0];
            af[s] = rz < NCLS + 2 ? v : 0.f;
        }
    }
    for (int i0 = tid; i0 < (TM ? kTmGroup : ng) * FC; i0 += NT) {
        // (time-major: a thread per (channel, slot), slots fastest -- 32 lanes read 4 channels x 8 neighbouring floats: no bank conflict)
        const int g = TM ? (i0 & 7) : i0 / FC, c = TM ? (i0 >> 3) : i0 - g * FC;
        if (TM && g >= ng) continue;
        const int i = g * FC + c;
        const float* row = TM ? fb + c * TP + g : fb + g * fsz + c * TP + kHalo;
        float v[FT];
#pragma unroll
        for (int t = 0; t < FT; ++t) v[t] = row[TS * t];
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < FT; ++t) s += v[t];
        pooled[i] = s / (float)FT;
    }
    __syncthreads();
    if (tid < 64) {
        const int g = min(r, ng - 1);
        float bf[FC / 4];
#pragma unroll
        for (int s = 0; s < FC / 4; ++s) bf[s] = pooled[g * FC + 4 * s + q];
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < FC / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[s], bf[s], acc, 0, 0, 0);
        // this lane: utterance r, outputs o = 4 q + reg (classes 0 .. NCLS-1, then the two range outputs)
        float mx = -3.0e38f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) if (4 * q + reg < NCLS) mx = fmaxf(mx, acc[reg]);       // (NCLS % 4 == 0 or not: per-lane test)
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float e[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) e[reg] = expf(acc[reg] - mx);
        // se = ((e_0 + e_1) + e_2) + ... in class order: row q adds its classes to the sum of rows < q
        float se = 0.f;
#pragma unroll
        for (int row = 0; row < (NCLS + 3) / 4; ++row) {
            const float prev = __shfl(se, (row > 0 ? (row - 1) * 16 : 0) + r);
            float cur = row > 0 ? prev : 0.f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) if (4 * row + reg < NCLS) cur += e[reg];
            if (q == row) se = cur;
        }
        se = __shfl(se, ((NCLS + 3) / 4 - 1) * 16 + r);
        if (r < ng) {
            const size_t n = (size_t)(n0 + r);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int o = 4 * q + reg;
                if (o < NCLS) {
                    a.logits[n * NCLS + o] = acc[reg];
                    a.probs[n * NCLS + o] = e[reg] / se;
                } else if (o < NCLS + 2 && a.ranges) {
                    a.ranges[n * 2 + (o - NCLS)] = 1.0f / (1.0f + expf(-acc[reg]));
                }
            }
        }
    }
    __syncthreads();
}

// Zero halos (4 + 4 floats) of the rows a static-shape layer is about to write: [ng][COUT] rows of TOUT + 8 floats; one thread per
// (row, side), four stores each (one thread per element: three times the index arithmetic, +6 us per launch).
template <int NT, int COUT, int TOUT>
__device__ __forceinline__ void fused_zero_halo(float* yout, const int out_sz, const int ng, const int tid_in) {
    constexpr int TPO = TOUT + 2 * kHalo;
    if (TCR_WHATIF(1024)) return;
    const int tid = tid_in + opaque_zero();
    for (int i = tid; i < ng * COUT * 2; i += NT) {
        const int row = i >> 1;
        const int g = row / COUT, co = row - g * COUT;
        float* p = yout + g * out_sz + co * TPO + ((i & 1) ? kHalo + TOUT : 0);
        p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; p[3] = 0.f;
    }
}

// ---- head: global average pool -> fc / fc2 -> softmax / sigmoid (tc_resnet.py:43-52), shared by the fused kernels ----
template <int NT>
__device__ __forceinline__ void fused_head(const FusedArgs& a, float* lds, const int n0, const int ng, const int tid) {
    {
        const float* fb = lds + a.buf_off[a.feat_buf];
        const int fsz = a.feat_sz, tp = a.feat_t + 2 * kHalo;
        float* pooled = lds + a.buf_off[(a.feat_buf + 1) % 3];         // any buffer other than the feature buffer
        for (int i = tid; i < ng * a.feat_c; i += NT) {
            const int g = i / a.feat_c, c = i - g * a.feat_c;
            const float* row = fb + g * fsz + c * tp + kHalo;
            float s = 0.f;
            for (int t = 0; t < a.feat_t; ++t) s += row[t];
            pooled[i] = s / (float)a.feat_t;
        }
        __syncthreads();
        float* lg = pooled + a.group * a.feat_c;                        // [ng][nc + 2]
        const int no = a.nc + 2;
        for (int i = tid; i < ng * no; i += NT) {
            const int g = i / no, o = i - g * no;
            const float* pv = pooled + g * a.feat_c;
            float s = 0.f;
            if (o < a.nc) {
                const float* wf = a.params + a.fc_off + o;
#pragma unroll 8
                for (int c = 0; c < a.feat_c; ++c) s = fmaf(pv[c], wf[(size_t)c * a.nc], s);
            } else {
                const float* wf = a.params + a.fc2_off + (o - a.nc);
#pragma unroll 8
                for (int c = 0; c < a.feat_c; ++c) s = fmaf(pv[c], wf[(size_t)c * 2], s);
            }
            lg[i] = s;
        }
        __syncthreads();
        // softmax / sigmoid: one thread per (utterance, output); the max and the sum are recomputed per thread
        // from the LDS row in the SAME order as the single-thread form (bitwise identical results)
        for (int i = tid; i < ng * no; i += NT) {
            const int g = i / no, o = i - g * no;
            const float* z = lg + g * no;
            const size_t n = (size_t)(n0 + g);
            if (o < a.nc) {
                float mx = z[0];
                for (int k = 1; k < a.nc; ++k) mx = fmaxf(mx, z[k]);
                float se = 0.f;
                for (int k = 0; k < a.nc; ++k) se += expf(z[k] - mx);
                a.logits[n * a.nc + o] = z[o];
                a.probs[n * a.nc + o] = expf(z[o] - mx) / se;
            } else if (a.ranges) {
                a.ranges[n * 2 + (o - a.nc)] = 1.0f / (1.0f + expf(-z[o]));
            }
        }
        __syncthreads();
    }
}

// TCResNet8-1.0 on 40 coefficients with every layer shape fixed at compile time (T0 = 49 or 98 frames): the flagship
// configurations of BASELINE.json.  Same walk, same LDS plan (FusedArgs), bitwise the generic kernel's results.
#define TCR_WAVES_PER_SIMD_4 TCR_WAVES_PER_SIMD(4)     // two 8-wave workgroups per CU: <= 128 VGPRs
// Row LI of the layer table, read WHERE the layer runs: the index carries an opaque wave-uniform zero, so the row's fields are scalar
// loads from the kernel-argument segment in front of the layer.  Indexed by the constant alone, every row of the table is loaded at the
// kernel's entry and held across the group loop -- more scalar registers than there are: they were spilled into VGPR lanes at the entry
// (v_writelane) and fetched back (v_readlane) inside the layers' loops.
// (AT: per instance -- the forms that fit their scalar registers without it keep the plain index, see profiles/net_valu_kernel_regs.txt)
#define TCR_LAYER_ROW(AT, LI) a.layer[(LI) + ((AT) ? __builtin_amdgcn_readfirstlane(opaque_zero()) : 0)]
// WD < 0: the round-2 layer (A/B arm, TCR_TUNE_NET_FUSED = 4).  HALO: some consumer convolves this layer's rows (K > 1) and so reads
// their zero halo; the shortcut convs' outputs (only ever a residual term) and the last block output (only pooled) skip the zero pass.
template <int NW, int K, int S, int CIN, int COUT, int TIN, int WD, bool HAS_RES, bool HALO = true, int NTJ = 2, bool WLDS = false>
__device__ __forceinline__ void fused_layer_sel(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                                float* lds, const int ng, const int wave, const int r, const int q,
                                                const int w_lds = 0) {
    if constexpr (WD < 0) fused_layer_t<NW, K, S, CIN, COUT, TIN>(a, L, xin, in_sz, lds, ng, wave, r, q);
    else {
        if constexpr (HALO) fused_zero_halo<NW * 64, COUT, (TIN + S - 1) / S>(lds + a.buf_off[L.out_buf], L.out_sz, ng, (int)threadIdx.x);
        if constexpr (NTJ == 0) fused_layer_u<NW, K, S, CIN, COUT, TIN, HAS_RES>(a, L, xin, in_sz, lds, ng, wave, r, q);      // (units: see fused_layer_u)
        else if constexpr (NTJ == 3) fused_layer_u<NW, K, S, CIN, COUT, TIN, HAS_RES, (CIN <= 32 ? 1 : 0)>(a, L, xin, in_sz, lds, ng, wave, r, q);   // (+ a whole tap of weight lookahead in the layers of <= 32 input channels)
        else if constexpr (NTJ == 13) fused_layer_u<NW, K, S, CIN, COUT, TIN, HAS_RES, (CIN <= 48 ? 1 : 0)>(a, L, xin, in_sz, lds, ng, wave, r, q);   // (TCResNet14-1.5's kernel: <= 48)
        else fused_layer_s<NW, K, S, CIN, COUT, TIN, HAS_RES, NTJ, WLDS>(a, L, xin, in_sz, lds, ng, wave, r, q, w_lds);
    }
}

// TM: the time-major plan (fused_layer_tm; the host lays the buffers out by the same fused_tm_pitch): groups of 8 at 49 frames, the default
// there; TCR_TUNE_NET_FUSED = 12 keeps the utterance-major walk.
// ONE table of the ten layers, in the order the walk runs them: fused_tc8_frames admits only a plan whose layers are these rows in this order, the
// image's layer order is the plan's (net.cpp), and the kernel's image offsets come from the same rows (fused_tc8_walk.inc calls layer LI with row LI's shape).
struct Tc8Shape { int k, stride, cin, cout; };
__host__ __device__ constexpr Tc8Shape tc8_shape(const int li) {
    constexpr Tc8Shape shape[10] = {{3, 1, 40, 16}, {1, 2, 16, 24}, {9, 2, 16, 24}, {9, 1, 24, 24}, {1, 2, 24, 32},
                                    {9, 2, 24, 32}, {9, 1, 32, 32}, {1, 2, 32, 48}, {9, 2, 32, 48}, {9, 1, 48, 48}};
    return shape[li];
}
// float offset of layer li's fragments in TCResNet8-1.0's weight image (li = 10: the image's size)
__host__ __device__ constexpr int tc8_wimg_off(const int li) {
    int n = 0;
    for (int i = 0; i < li && i < 10; ++i) n += wimg_layer_floats(tc8_shape(i).k, tc8_shape(i).cin, tc8_shape(i).cout);
    return n;
}

// The kernel's walk is ONE text, fused_tc8_walk.inc, compiled as the kernel itself (weights from `params`: every instance but the one below)
// and as a function with IMG as a parameter for the instance that chooses per launch.  (All of them calling the function cost the
// utterance-major instances 8 B of scratch: a function's code is simplified before it is inlined, without the kernel's workgroup size.)
template <int NW, int T0, int WD, int NTJ0 = 2, bool TM = false>
__global__ __launch_bounds__(NW * 64) TCR_WAVES_PER_SIMD_4 void net_fused_tc8_kernel(const FusedArgs a) {
    constexpr bool IMG = false;
#include "fused_tc8_walk.inc"
}
// IMG: the weight fragments, scale and shift come out of the frozen table's fragment-ordered image.
template <int NW, int T0, int WD, int NTJ0, bool TM, bool IMG>
__device__ __forceinline__ void net_fused_tc8_walk(const FusedArgs& a) {
#include "fused_tc8_walk.inc"
}
// The time-major instance reads the table's weight image where a launch finds it valid (both walks are compiled in; the test is
// wave-uniform, once per launch), `params` otherwise.  (An overload of the kernel template: six arguments, the last one WIMG = true.)
template <int NW, int T0, int WD, int NTJ0, bool TM, bool WIMG>
__global__ __launch_bounds__(NW * 64) TCR_WAVES_PER_SIMD_4 void net_fused_tc8_kernel(const FusedArgs a) {
    static_assert(TM && WIMG, "the instance with a weight image is the time-major one");
    if (wimg_present(a)) net_fused_tc8_walk<NW, T0, WD, NTJ0, TM, true>(a);
    else net_fused_tc8_walk<NW, T0, WD, NTJ0, TM, false>(a);
}

// Small-batch (latency) form of the same network, TCResNet8-1.0 at 49 frames: ONE utterance per 8-wave workgroup, every phase's weights
// copied into LDS by the DMA path (global_load_lds_dwordx4, coalesced, all in flight at once) one phase ahead, A fragments read from
// LDS.  In the throughput kernel a job's nine taps are nine DEPENDENT weight loads from L2 (cold L1 at batch 1): ~4.5 us per layer,
// 35 us for the walk; here a phase costs one L2 round trip, hidden behind the phase before it (two weight buffers: 83 KB + 61 KB, the
// two largest consecutive phases).  One 16-position tile per job: more jobs for the eight waves, half the matrix work of a
// two-tile job whose second tile would be empty at 13 / 7 frames.  Same accumulation order as the throughput kernels: bitwise their
// results, so an utterance's outputs do not depend on the batch it arrives in.  (Round 4's `net_small_kernel` -- every weight fragment of
// a job gathered into registers -- was slower than the throughput kernel: 108 dword gathers per lane and job.)
template <int NW>
__device__ __forceinline__ void small_stage_weights(const float* __restrict__ src, int n_floats, float* dst, int wave, int lane) {
    for (int c0 = wave * 256; c0 < n_floats; c0 += NW * 256) {          // one DMA instruction: 64 lanes x 16 B = 256 floats
        const int c = c0 + 4 * lane;
        if (c < n_floats) glds16(src + c, dst + c0);
    }
}

template <int NW, int T0>
__global__ __launch_bounds__(NW * 64) void net_small_tc8_kernel(const FusedArgs a, const int wa_off, const int wb_off) {
    constexpr int NT = NW * 64;
    constexpr int T1 = (T0 + 1) / 2, T2 = (T1 + 1) / 2, T3 = (T2 + 1) / 2;
    float* lds = reinterpret_cast<float*>(dyn_lds());
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int row = a.in_c * a.in_tp;
    float* WA = lds + wa_off;
    float* WB = lds + wb_off;
    constexpr int W0 = 3 * 40 * 16, WD0 = 16 * 24, W00 = 9 * 16 * 24, W01 = 9 * 24 * 24, WD1 = 24 * 32, W10 = 9 * 24 * 32, W11 = 9 * 32 * 32,
                  WD2 = 32 * 48, W20 = 9 * 32 * 48, W21 = 9 * 48 * 48;
#define TCR_SM_W(LI) (a.params + a.layer[LI].w_off)
#define TCR_SM(LI, K_, S_, CI_, CO_, T_, WP_) fused_layer_sel<NW, K_, S_, CI_, CO_, T_, 0, (LI == 3 || LI == 6 || LI == 9), (K_ != 1 && LI != 9), 1, true>(a, a.layer[LI], lds + a.buf_off[a.layer[LI].in_buf], a.layer[LI].in_sz, lds, 1, wave, r, q, WP_)
#if TCR_FUSED_WHATIF & 2048
    long long ts[16];
    int nts = 0;
#define TCR_SM_TS() ts[nts++] = (long long)__builtin_readcyclecounter()
#else
#define TCR_SM_TS() ((void)0)
#endif
    for (int n0 = blockIdx.x; n0 < a.batch; n0 += gridDim.x) {
        TCR_SM_TS();
        small_stage_weights<NW>(TCR_SM_W(0), W0, WA, wave, lane);               // phase 0 -> A
        small_stage_weights<NW>(TCR_SM_W(1), WD0, WB, wave, lane);              // phase 1 -> B
        small_stage_weights<NW>(TCR_SM_W(2), W00, WB + WD0, wave, lane);
        fused_zero_halo<NT, 16, T0>(lds + a.buf_off[a.layer[0].out_buf], a.layer[0].out_sz, 1, tid);
        wait_dma();
        __syncthreads();
        TCR_SM_TS();
        fused_conv0_s<NW, T0, true>(a, a.layer[0], a.feat + (size_t)n0 * row, row, lds, 1, wave, r, q, wa_off);
        __syncthreads();
        TCR_SM_TS();
        small_stage_weights<NW>(TCR_SM_W(3), W01, WA, wave, lane);              // phase 2 -> A (conv0 is done with it)
        TCR_SM(1, 1, 2, 16, 24, T0, wb_off);
        TCR_SM(2, 9, 2, 16, 24, T0, wb_off + WD0);
        wait_dma();
        __syncthreads();
        TCR_SM_TS();
        small_stage_weights<NW>(TCR_SM_W(4), WD1, WB, wave, lane);              // phase 3 -> B
        small_stage_weights<NW>(TCR_SM_W(5), W10, WB + WD1, wave, lane);
        TCR_SM(3, 9, 1, 24, 24, T1, wa_off);
        wait_dma();
        __syncthreads();
        TCR_SM_TS();
        small_stage_weights<NW>(TCR_SM_W(6), W11, WA, wave, lane);              // phase 4 -> A
        TCR_SM(4, 1, 2, 24, 32, T1, wb_off);
        TCR_SM(5, 9, 2, 24, 32, T1, wb_off + WD1);
        wait_dma();
        __syncthreads();
        TCR_SM_TS();
        small_stage_weights<NW>(TCR_SM_W(7), WD2, WB, wave, lane);              // phase 5 -> B
        small_stage_weights<NW>(TCR_SM_W(8), W20, WB + WD2, wave, lane);
        TCR_SM(6, 9, 1, 32, 32, T2, wa_off);
        wait_dma();
        __syncthreads();
        TCR_SM_TS();
        small_stage_weights<NW>(TCR_SM_W(9), W21, WA, wave, lane);              // phase 6 -> A
        TCR_SM(7, 1, 2, 32, 48, T2, wb_off);
        TCR_SM(8, 9, 2, 32, 48, T2, wb_off + WD2);
        wait_dma();
        __syncthreads();
        TCR_SM_TS();
        TCR_SM(9, 9, 1, 48, 48, T3, wa_off);
        __syncthreads();
        TCR_SM_TS();
        if (a.nc == 12) fused_head_s<NT, 48, T3, 12>(a, lds, n0, 1, tid);
        else fused_head<NT>(a, lds, n0, 1, tid);
#if TCR_FUSED_WHATIF & 2048
        __syncthreads();
        TCR_SM_TS();
        if (tid == 0)
            for (int i = 0; i + 1 < nts && i < 12; ++i) a.probs[(size_t)n0 * a.nc + i] = (float)(ts[i + 1] - ts[i]);
        nts = 0;
#endif
    }
#undef TCR_SM
#undef TCR_SM_W
#undef TCR_SM_TS
}

// TCResNet14-1.5 (channels 24 / 36 / 36 / 48 / 48 / 72 / 72; BASELINE.json configs[3]'s network) with compile-time layer shapes, T0 = 49 or 98
// frames: the same static layer (`fused_layer_s`), first conv (`fused_conv0_g`: 24 output channels = two row tiles) and head as the
// TCResNet8 instance.  Blocks 1 / 3 / 5 have identity shortcuts: their second conv adds the block input, which lives in its own output
// buffer (each lane reads the residual of exactly the elements it then writes).
template <int NW, int T0, int NTJ0 = 13>      // NTJ0: the nine-tap layers as in net_fused_tc8_kernel (13: units + weight lookahead up to 48 input channels, 0: units, 2: jobs of two tiles)
__global__ __launch_bounds__(NW * 64) TCR_WAVES_PER_SIMD_4 void net_fused_tc14w_kernel(const FusedArgs a) {
    constexpr int NT = NW * 64;
    constexpr int T1 = (T0 + 1) / 2, T2 = (T1 + 1) / 2, T3 = (T2 + 1) / 2;
    float* lds = reinterpret_cast<float*>(dyn_lds());
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int row = a.in_c * a.in_tp;
#define TCR_L(LI, K_, S_, CI_, CO_, T_, RES_, HALO_) do { const FusedLayer& L_ = TCR_LAYER_ROW(NTJ0 == 13, LI); \
        fused_layer_sel<NW, K_, S_, CI_, CO_, T_, 0, RES_, HALO_, (K_ == 9 ? NTJ0 : 2)>(a, L_, lds + a.buf_off[L_.in_buf], L_.in_sz, lds, ng, wave, r, q); } while (0)
    for (int grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
        const int n0 = grp * a.group;
        const int ng = min(a.group, a.batch - n0);
        fused_zero_halo<NT, 24, T0>(lds + a.buf_off[a.layer[0].out_buf], a.layer[0].out_sz, ng, tid);
        fused_conv0_g<NW>(a, a.layer[0], a.feat + (size_t)n0 * row, row, lds, ng, wave, r, q);
        __syncthreads();
        TCR_L(1, 1, 2, 24, 36, T0, false, false);       // block0: shortcut conv + first conv (same input rows: one phase)
        TCR_L(2, 9, 2, 24, 36, T0, false, true);
        __syncthreads();
        TCR_L(3, 9, 1, 36, 36, T1, true, true);
        __syncthreads();
        TCR_L(4, 9, 1, 36, 36, T1, false, true);        // block1 (identity shortcut)
        __syncthreads();
        TCR_L(5, 9, 1, 36, 36, T1, true, true);
        __syncthreads();
        TCR_L(6, 1, 2, 36, 48, T1, false, false);       // block2
        TCR_L(7, 9, 2, 36, 48, T1, false, true);
        __syncthreads();
        TCR_L(8, 9, 1, 48, 48, T2, true, true);
        __syncthreads();
        TCR_L(9, 9, 1, 48, 48, T2, false, true);        // block3 (identity)
        __syncthreads();
        TCR_L(10, 9, 1, 48, 48, T2, true, true);
        __syncthreads();
        TCR_L(11, 1, 2, 48, 72, T2, false, false);      // block4
        TCR_L(12, 9, 2, 48, 72, T2, false, true);
        __syncthreads();
        TCR_L(13, 9, 1, 72, 72, T3, true, true);
        __syncthreads();
        TCR_L(14, 9, 1, 72, 72, T3, false, true);       // block5 (identity)
        __syncthreads();
        TCR_L(15, 9, 1, 72, 72, T3, true, false);
        __syncthreads();
        if (a.nc == 12) fused_head_s<NT, 72, T3, 12>(a, lds, n0, ng, tid);
        else fused_head<NT>(a, lds, n0, ng, tid);
    }
#undef TCR_L
}

// 49 / 98 when the plan is exactly TCResNet14-1.5 on 40 coefficients read from global memory, else 0
static int fused_tc14w_frames(const FusedArgs& a) {
    static const int shape[16][4] = {{3, 1, 40, 24}, {1, 2, 24, 36}, {9, 2, 24, 36}, {9, 1, 36, 36}, {9, 1, 36, 36}, {9, 1, 36, 36}, {1, 2, 36, 48}, {9, 2, 36, 48},
                                     {9, 1, 48, 48}, {9, 1, 48, 48}, {9, 1, 48, 48}, {1, 2, 48, 72}, {9, 2, 48, 72}, {9, 1, 72, 72}, {9, 1, 72, 72}, {9, 1, 72, 72}};
    if (a.n_layers != 16 || !a.in_global || a.in_c != 40) return 0;
    const int t0 = a.layer[0].tin;
    if (t0 != 49 && t0 != 98) return 0;
    int t = t0;
    for (int i = 0; i < 16; ++i) {
        const FusedLayer& L = a.layer[i];
        if (L.k != shape[i][0] || L.stride != shape[i][1] || L.cin != shape[i][2] || L.cout != shape[i][3] || L.tin != t) return 0;
        if (i == 2 || i == 7 || i == 12) t = (t + 1) / 2;
    }
    return t0;
}

static int fused_tc8_frames(const FusedArgs& a);
// The time-major plan has ONE kernel instance: TCResNet8-1.0 at 49 frames and 12 classes, groups of 8, 8 waves, the default arm.
bool fused_tmajor_applies(const FusedArgs& a, const int waves) {
    return (tune_get(TCR_TUNE_NET_FUSED) == 0 || tune_get(TCR_TUNE_NET_FUSED) == 13) && a.group == kTmGroup && waves == 8 && a.nc == 12 && fused_tc8_frames(a) == 49;
}
// the kernel derives every pitch at compile time from the layer shapes; the host derived them from the plan's actual readers
static bool fused_tmajor_pitches_agree(const FusedArgs& a) {
    for (int i = 0; i < a.n_layers; ++i) {
        const FusedLayer& L = a.layer[i];
        const int ocs = (L.k == 1 || i == a.n_layers - 1) ? 0 : (L.stride == 2 ? 1 : 2);
        if (L.out_sz != fused_tm_pitch(L.tout, ocs != 0, ocs)) return false;
        if (i > 0 && L.in_sz != fused_tm_pitch(L.tin, true, L.stride)) return false;
        if (L.res_buf >= 0 && L.res_sz != fused_tm_pitch(L.tout, false, 0)) return false;
        if (L.pad_lo != (L.k == 9 ? 4 : L.k == 3 ? 1 : 0)) return false;
    }
    return a.feat_sz == fused_tm_pitch(a.feat_t, false, 0);
}

// 49 / 98 when the plan is exactly TCResNet8-1.0 on 40 coefficients read from global memory, else 0
static int fused_tc8_frames(const FusedArgs& a) {
    if (a.n_layers != 10 || !a.in_global || a.in_c != 40) return 0;
    const int t0 = a.layer[0].tin;
    if (t0 != 49 && t0 != 98) return 0;
    int t = t0;
    for (int i = 0; i < 10; ++i) {
        const FusedLayer& L = a.layer[i];
        const Tc8Shape sh = tc8_shape(i);
        if (L.k != sh.k || L.stride != sh.stride || L.cin != sh.cin || L.cout != sh.cout || L.tin != t) return 0;
        if (i == 2 || i == 5 || i == 8) t = (t + 1) / 2;
    }
    return t0;
}

// Runtime-shape twins of fused_zero_halo / fused_conv0_s / fused_head_s for the generic walk (TCResNet14, other widths).
template <int NT>
__device__ __forceinline__ void fused_zero_halo_g(float* yout, const int out_sz, const int ng, const int cout, const int tout, const int tid_in) {
    const int tpo = tout + 2 * kHalo;
    const int tid = tid_in + opaque_zero();
    const float inv = 1.0f / (float)cout;
    for (int i = tid; i < ng * cout * 2; i += NT) {
        const int row = i >> 1;
        const int g = fast_div(row, cout, inv), co = row - g * cout;
        float* p = yout + g * out_sz + co * tpo + ((i & 1) ? kHalo + tout : 0);
        p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; p[3] = 0.f;
    }
}

// first conv (3 x 1, stride 1, 40 input channels) from global memory with every operand of a job requested up front
template <int NW>
__device__ __forceinline__ void fused_conv0_g(const FusedArgs& a, const FusedLayer& L, const float* __restrict__ xin, const int in_sz,
                                              float* lds, const int ng, const int wave, const int r_in, const int q_in) {
    constexpr int K = 3, C4 = 10, PADLO = 1;
    const int oz = opaque_zero();
    const int r = r_in + oz, q = q_in + oz;
    const int cout = L.cout, tout = L.tout, tpi = L.tin + 2 * kHalo, tpo = tout + 2 * kHalo;
    const int wstep = 4 * cout, xstep = 4 * tpi;
    float* yout = lds + a.buf_off[L.out_buf];
    const int out_sz = L.out_sz;
    const int npos = ng * tout;
    const int nct = (npos + 15) / 16, nrt = (cout + 15) / 16;
    const float* w = a.params + L.w_off;
    const float* scale = a.ss + L.ss_off;
    const float* shift = scale + L.c_pad;
    const float inv_tout = 1.0f / (float)tout;
    for (int job = wave; job < nct * nrt; job += NW) {
        const int ct = job / nrt, m = job - ct * nrt;
        const int p0 = min(ct * 16 + r, npos - 1);
        const int g0 = fast_div(p0, tout, inv_tout);
        const int t0 = p0 - g0 * tout;
        const float* wp = w + q * cout + min(m * 16 + r, cout - 1);
        const float* x0 = xin + g0 * in_sz + q * tpi + t0 + kHalo - PADLO;
        float b0[C4][K], wf[K][C4];
#pragma unroll
        for (int c4 = 0; c4 < C4; ++c4)
#pragma unroll
            for (int j = 0; j < K; ++j) b0[c4][j] = x0[c4 * xstep + j];
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4) wf[j][c4] = wp[(j * C4 + c4) * wstep];
        float sc[4], sh[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int co = min(m * 16 + q * 4 + reg, cout - 1);
            sc[reg] = scale[co];
            sh[reg] = shift[co];
        }
        f32x4 acc0 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[j][c4], b0[c4][j], acc0, 0, 0, 0);
        const int dump = a.buf_off[2] + a.group * a.buf_sz[2] + (q * 16 + r) - a.buf_off[L.out_buf];
        const float lo = L.relu ? 0.f : -3.4e38f;
        const bool pv = ct * 16 + r < npos;
        const int base = g0 * out_sz + kHalo + t0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int co = m * 16 + q * 4 + reg;
            const float v = fmaxf(fmaf(acc0[reg], sc[reg], sh[reg]), lo);
            yout[(pv && co < cout) ? base + co * tpo : dump] = v;
        }
    }
}

// head with runtime shapes: pool by all threads, fc / fc2 + softmax by one wave on the matrix cores (feat_c % 4 == 0, nc <= 14)
template <int NT>
__device__ __forceinline__ void fused_head_g(const FusedArgs& a, float* lds, const int n0, const int ng, const int tid_in) {
    const int tid = tid_in + opaque_zero();
    const int fc = a.feat_c, ft = a.feat_t, nc = a.nc;
    const int tp = ft + 2 * kHalo;
    const float* fb = lds + a.buf_off[a.feat_buf];
    const int fsz = a.feat_sz;
    float* pooled = lds + a.buf_off[(a.feat_buf + 1) % 3];
    const int lane = tid & 63, r = lane & 15, q = lane >> 4;
    const float inv_fc = 1.0f / (float)fc;
    for (int i = tid; i < ng * fc; i += NT) {
        const int g = fast_div(i, fc, inv_fc), c = i - g * fc;
        const float* row = fb + g * fsz + c * tp + kHalo;
        float s = 0.f;
        for (int t = 0; t < ft; ++t) s += row[t];
        pooled[i] = s / (float)ft;
    }
    __syncthreads();
    if (tid < 64) {
        const int g = min(r, ng - 1);
        const float* wsrc = r < nc ? a.params + a.fc_off + r : a.params + a.fc2_off + min(r - nc, 1);
        const int wstride = r < nc ? nc : 2;
        const bool wv = r < nc + 2;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        const int nst = fc >> 2;
        for (int s0 = 0; s0 < nst; s0 += 6) {           // six K-steps per trip: their 6 + 6 operand loads in flight together
            float af[6], bf[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int c = 4 * min(s0 + i, nst - 1) + q;
                af[i] = wsrc[c * wstride];
                bf[i] = pooled[g * fc + c];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i)
                if (s0 + i < nst) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv ? af[i] : 0.f, bf[i], acc, 0, 0, 0);
        }
        float mx = -3.0e38f;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) if (4 * q + reg < nc) mx = fmaxf(mx, acc[reg]);
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float e[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) e[reg] = expf(acc[reg] - mx);
        float se = 0.f;
#pragma unroll
        for (int row = 0; row < 4; ++row) {             // class sum carried through the 16-lane rows in class order
            const float prev = __shfl(se, (row > 0 ? (row - 1) * 16 : 0) + r);
            float cur = row > 0 ? prev : 0.f;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) if (4 * row + reg < nc) cur += e[reg];
            if (q == row) se = cur;
        }
        se = __shfl(se, 48 + r);
        if (r < ng) {
            const size_t n = (size_t)(n0 + r);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int o = 4 * q + reg;
                if (o < nc) {
                    a.logits[n * nc + o] = acc[reg];
                    a.probs[n * nc + o] = e[reg] / se;
                } else if (o < nc + 2 && a.ranges) {
                    a.ranges[n * 2 + (o - nc)] = 1.0f / (1.0f + expf(-acc[reg]));
                }
            }
        }
    }
    __syncthreads();
}

template <int NW, int R>
__global__ __launch_bounds__(NW * 64) void net_fused_kernel(const FusedArgs a) {
    constexpr int NT = NW * 64;
    float* lds = reinterpret_cast<float*>(dyn_lds());
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // uniform: job bookkeeping runs on the scalar unit
    const int r = lane & 15, q = lane >> 4;

    for (int grp = blockIdx.x; grp < a.n_groups; grp += gridDim.x) {
        const int n0 = grp * a.group;
        const int ng = min(a.group, a.batch - n0);
        const int row = a.in_c * a.in_tp;
        if (!a.in_global) {
            // ---- stage the group's feature rows (contiguous in global memory) ----
            const float4* src = reinterpret_cast<const float4*>(a.feat + (size_t)n0 * row);
            float4* dst = reinterpret_cast<float4*>(lds + a.buf_off[0]);
            const int nvec = ng * row / 4;
            for (int i = tid; i < nvec; i += NT) dst[i] = src[i];
            __syncthreads();
        }

        for (int li = 0; li < a.n_layers; ++li) {
            const FusedLayer L = a.layer[li];
            fused_zero_halo_g<NT>(lds + a.buf_off[L.out_buf], L.out_sz, ng, L.cout, L.tout, tid);
            if (li == 0 && a.in_global) {
                if (L.k == 3 && L.cin == 40 && L.stride == 1 && L.pad_lo == 1) fused_conv0_g<NW>(a, L, a.feat + (size_t)n0 * row, row, lds, ng, wave, r, q);
                else fused_layer<NW, R>(a, L, a.feat + (size_t)n0 * row, row, lds, ng, wave, r, q);
            } else {
                fused_layer<NW, R>(a, L, lds + a.buf_off[L.in_buf], L.in_sz, lds, ng, wave, r, q);
            }
            if (!L.no_barrier) __syncthreads();         // (a block's shortcut conv and its first conv read the same input: one phase)
        }

        if ((a.feat_c & 3) == 0 && a.nc + 2 <= 16) fused_head_g<NT>(a, lds, n0, ng, tid);
        else fused_head<NT>(a, lds, n0, ng, tid);
    }
}

// one utterance per group, TCResNet8-1.0 at 49 frames, few utterances: the small-batch kernel (weights through LDS); 1: not taken
static int launch_net_small(const FusedArgs& a0, hipStream_t s) {
    constexpr int kWA = 9 * 48 * 48, kWB = 32 * 48 + 9 * 32 * 48;       // the two largest consecutive phases: conv2_1 | down2 + conv2_0
    FusedArgs a = a0;
    // the weight copies are 16-byte DMA reads (global_load_lds_dwordx4) at params + w_off: a C-ABI caller's arena aligned to 4 bytes only
    // (or a layer whose weights do not start on a 16-byte boundary) takes the throughput kernel instead (advisor, round 5)
    if (reinterpret_cast<uintptr_t>(a.params) % 16 != 0) return 1;
    for (int li = 0; li < a.n_layers; ++li)
        if (a.layer[li].w_off % 4 != 0) return 1;
    const int act = a.buf_off[2] + a.buf_sz[2];                         // group == 1
    const int wa_off = (act + 64 + 63) / 64 * 64, wb_off = wa_off + kWA + 64;      // (+ pad: the layers' one-step operand lookahead)
    const size_t lds = ((size_t)wb_off + kWB + 64) * sizeof(float);
    if (lds > 160 * 1024) return 1;
    static bool configured = false;
    if (!configured) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(net_small_tc8_kernel<8, 49>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
            (void)hipGetLastError();
            return 1;
        }
        configured = true;
    }
    hipLaunchKernelGGL((net_small_tc8_kernel<8, 49>), dim3(a.batch), dim3(512), lds, s, a, wa_off, wb_off);
    return check_launch("net_small_tc8_kernel");
}

int launch_net_fused(const FusedArgs& a, size_t lds_bytes, int grid, int waves, int ring, hipStream_t s) {
    void (*kern)(const FusedArgs) = nullptr;
    const int tc8 = tune_get(TCR_TUNE_NET_FUSED) == 3 ? 0 : fused_tc8_frames(a);
    if (tc8 == 49 && a.group == 1 && a.batch <= kSmallBatchMax && a.nc + 2 <= 16 && tune_get(TCR_TUNE_NET_FUSED) == 0 && tune_get(TCR_TUNE_NET_SMALL) == 0 &&
        tune_get(TCR_TUNE_FUSED_WAVES) == 0) {
        const int rc = launch_net_small(a, s);
        if (rc != 1) return rc;
    }
    // TCR_TUNE_NET_FUSED: 0 branch-free epilogue (default); 4: the round-2 static-shape kernel (A/B arm)
    const bool r2 = tune_get(TCR_TUNE_NET_FUSED) == 4;
    // Round 6 default: the nine-tap layers' work dealt in 16-position units (fused_layer_u) + a whole tap of weight lookahead (fused_job_s AHEAD) in
    // the layers of <= 24 input channels: 105.1 -> 98.6 -> 95.3 us at 49 frames, 182 -> 178 -> 175 at 98, bitwise; <= 32: 96.4 -> 95.3 / 178.3 -> 173.4;
    // every width: 96.5 (128 registers + 156 B of scratch).  TCResNet14-1.5's kernel: <= 48 input channels (98 frames 837 -> 804 us, 49 frames
    // 423.6 -> 421.7; 224 B of scratch).  A/B arms: 8 the jobs of two tiles dealt round-robin (rounds 3-5), 9 units without the lookahead.
    const bool j2 = tune_get(TCR_TUNE_NET_FUSED) == 8;
    const bool ju = tune_get(TCR_TUNE_NET_FUSED) == 9;
    const bool j4 = tune_get(TCR_TUNE_NET_FUSED) == 5;         // 5: four 16-position tiles per job in block 0's layers (A/B arm, bitwise; measured 103.6 vs 103.2 us at 49 frames, 184.9 vs 181.2 at 98: no gain)
    // conv0_1's weights resident in registers across a wave's run of units (fused_layer_r): the default at 49 frames (kernel alone 107.4 - 108.5 ->
    // 106.0 - 106.3 us); at 98 frames it measured no faster (186.5 - 188.1 against 185.7 - 186.1 us) and the round-6 walk stays.  A/B arms (bitwise):
    // 10 the round-6 walk (a tap of weight lookahead per job) in that layer too, 11 the resident walk at either frame count.
    const bool jl = tune_get(TCR_TUNE_NET_FUSED) == 10;
    const bool jr = tune_get(TCR_TUNE_NET_FUSED) == 11;
#define TCR_FS(NW_, T_) if (tc8 == T_ && waves == NW_) kern = r2 ? net_fused_tc8_kernel<NW_, T_, -1> : (j4 ? net_fused_tc8_kernel<NW_, T_, 0, 4> : (ju ? net_fused_tc8_kernel<NW_, T_, 0, 0> : (j2 ? net_fused_tc8_kernel<NW_, T_, 0, 2> : ((jr || (T_ == 49 && !jl)) ? net_fused_tc8_kernel<NW_, T_, 0, 6> : net_fused_tc8_kernel<NW_, T_, 0, 3>))));
    TCR_FS(4, 49) TCR_FS(8, 49) TCR_FS(16, 49) TCR_FS(4, 98) TCR_FS(8, 98) TCR_FS(16, 98)
#undef TCR_FS
    if (a.tmajor) {
        // the host laid the buffers out time-major (fused_tmajor_applies held): the one instance built for it, or an error -- never the other walk on these rows
        if (!fused_tmajor_applies(a, waves) || !fused_tmajor_pitches_agree(a)) { set_error("fused kernel: time-major plan without its kernel instance"); return TCR_ERR_ARG; }
        // The instance that takes its weight fragments out of the frozen table's image where the table carries a valid one (the kernel tests the
        // header); TCR_TUNE_NET_FUSED = 13: the dword loads from `params` whatever the table carries (A/B arm, bitwise).  The image's layout is fixed
        // by the layer shapes, compiled into the kernel: a plan that sizes it differently is refused.
        constexpr int kImg = tc8_wimg_off(10);
        if (a.wimg_floats != kImg) { set_error("fused kernel: the plan's weight image has %d floats, the kernel's %d", a.wimg_floats, kImg); return TCR_ERR_ARG; }
        if (a.wimg && reinterpret_cast<uintptr_t>(a.wimg) % 16 != 0) { set_error("fused kernel: the frozen table's weight image is not on a 16-byte boundary"); return TCR_ERR_ARG; }
        kern = tune_get(TCR_TUNE_NET_FUSED) == 13 ? net_fused_tc8_kernel<8, 49, 0, 6, true> : net_fused_tc8_kernel<8, 49, 0, 6, true, true>;
    }
    const int tc14 = (kern || tune_get(TCR_TUNE_NET_FUSED) == 3 || tune_get(TCR_TUNE_NET_FUSED) == 4) ? 0 : fused_tc14w_frames(a);
#define TCR_F14(NW_, T_) if (tc14 == T_ && waves == NW_) kern = ju ? net_fused_tc14w_kernel<NW_, T_, 0> : (j2 ? net_fused_tc14w_kernel<NW_, T_, 2> : net_fused_tc14w_kernel<NW_, T_, 13>);
    TCR_F14(8, 49) TCR_F14(16, 49) TCR_F14(8, 98) TCR_F14(16, 98)
#undef TCR_F14
    if (kern) ring = 0;
#define TCR_FK(NW_, R_) if (!kern && waves == NW_ && ring == R_) kern = net_fused_kernel<NW_, R_>;
    TCR_FK(4, 4) TCR_FK(4, 8) TCR_FK(4, 16) TCR_FK(8, 4) TCR_FK(8, 8) TCR_FK(8, 16) TCR_FK(16, 4) TCR_FK(16, 8) TCR_FK(16, 16)
#undef TCR_FK
    if (!kern) { set_error("fused kernel: no instantiation for %d waves / ring %d", waves, ring); return TCR_ERR_ARG; }
    if (lds_bytes > 64 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return 1;       // caller falls back to the per-layer kernels
        }
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(waves * 64), lds_bytes, s, a);
    return check_launch("net_fused_kernel");
}

// Frozen table's weight image (kernels.h "weight image"): one thread per float of the image gathers its weight; thread 0 then writes the header.
__global__ __launch_bounds__(256) void wimg_fold_kernel(const WimgFoldArgs a) {
    float* img = a.header + kWimgHeader;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < a.total; e += gridDim.x * 256) {
        int li = 0;
        while (li + 1 < a.n && e >= a.img_off[li + 1]) ++li;
        const int k = a.k[li], cin = a.cin[li], cout = a.cout[li], C4 = cin >> 2;
        const int x0 = e - a.img_off[li];
        const int per = k * C4 * 64;
        const int m = x0 / per, x1 = x0 - m * per;
        const int j = x1 / (C4 * 64), x2 = x1 - j * (C4 * 64);
        const int g = x2 >> 8, wd = min(4, C4 - 4 * g), y = x2 - (g << 8);
        const int lane = y / wd, c4 = 4 * g + (y - lane * wd);
        const int q = lane >> 4, r = lane & 15;
        img[e] = a.params[(size_t)a.w_off[li] + (size_t)((j * C4 + c4) * 4 + q) * cout + min(16 * m + r, cout - 1)];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned* h = reinterpret_cast<unsigned*>(a.header);
        h[0] = kWimgMagic; h[1] = (unsigned)a.total; h[2] = 0u; h[3] = 0u;
    }
}

int launch_wimg_fold(const WimgFoldArgs& a, hipStream_t s) {
    if (a.n < 1 || a.total < 1) { set_error("weight image: nothing to fold"); return TCR_ERR_ARG; }
    const int grid = min((a.total + 255) / 256, 1024);
    hipLaunchKernelGGL(wimg_fold_kernel, dim3(grid), dim3(256), 0, s, a);
    return check_launch("wimg_fold_kernel");
}

}  // namespace tcr

extern "C" int tcr_fused_tm_taps(int k, int stride, int tin, int pad_lo, int tile, int* out2) {
    if (!out2 || k < 1 || stride < 1 || tin < 1 || pad_lo < 0 || tile < 0 || 2 * tile >= (tin + stride - 1) / stride) {
        tcr::set_error("tcr_fused_tm_taps: bad arguments (k %d, stride %d, %d frames, tile %d)", k, stride, tin, tile);
        return TCR_ERR_ARG;
    }
    const tcr::FusedTaps t = tcr::fused_tm_taps(k, stride, tin, pad_lo, tile);
    out2[0] = t.lo; out2[1] = t.hi;
    return TCR_OK;
}

extern "C" int tcr_fused_tm_deal(int k, int stride, int cin, int cout, int tin, int pad_lo, int nw, int wave, unsigned* jobs, int cap, int* mfma) {
    if (!jobs || k < 1 || stride < 1 || cin < 4 || cout < 1 || cout > 256 || tin < 1 || tin > 126 || (nw != 4 && nw != 8 && nw != 16) || wave < 0 || wave >= nw || cap < tcr::kTmMaxJobs) {
        tcr::set_error("tcr_fused_tm_deal: bad arguments");
        return TCR_ERR_ARG;
    }
    const int tout = (tin + stride - 1) / stride;
    if (((cout + 15) / 16) * ((tout + 1) / 2) > nw * tcr::kTmMaxJobs) { tcr::set_error("tcr_fused_tm_deal: more jobs than the table holds"); return TCR_ERR_ARG; }
    const tcr::FusedTmDeal d = tcr::fused_tm_deal(k, stride, cin, cout, tin, pad_lo, nw);
    if (d.n[wave] > tcr::kTmMaxJobs) { tcr::set_error("tcr_fused_tm_deal: more jobs than the table holds"); return TCR_ERR_ARG; }
    for (int i = 0; i < d.n[wave]; ++i) jobs[i] = d.job[wave][i];
    if (mfma) *mfma = d.mfma;
    return d.n[wave];
}

extern "C" int tcr_fused_deal_run(int nrt, int nt16, int nw, int wave, int* out3) {
    if (!out3 || nrt < 1 || nt16 < 0 || nw < nrt || nw % nrt != 0 || wave < 0 || wave >= nw) {
        tcr::set_error("tcr_fused_deal_run: bad arguments (%d row tiles, %d column tiles, wave %d of %d)", nrt, nt16, wave, nw);
        return TCR_ERR_ARG;
    }
    const tcr::FusedRun run = tcr::fused_deal_run(nrt, nt16, nw, wave);
    out3[0] = run.m; out3[1] = run.c0; out3[2] = run.c1;
    return TCR_OK;
}
