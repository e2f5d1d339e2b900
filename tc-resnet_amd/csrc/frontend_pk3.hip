// Packed-FP32 fused MFCC / log-mel front-end at THREE waves per SIMD (the arithmetic of frontend_pk.hip, its decomposition in
// frontend.hip; reference semantics: datasets/preprocessors.py:64-96,183-194).
//
// frontend_pk.hip holds 245 VGPRs and 78.8 KB of LDS per 4-wave workgroup: two waves per SIMD, VALU 47 % and LDS 46 % busy, a quarter
// of the wave-cycles waiting (profiles/r04_final_pmc.csv).  This build fits three workgroups per CU -- <= 168 VGPRs, <= 53 KB:
//   * every LDS region is WAVE-LOCAL (a wave owns its frames from the samples to the DCT): one workgroup barrier in the kernel's life
//     (the slope table), the waves of a workgroup drift apart and cover each other's LDS / memory round trips;
//   * the 16 x 16 transpose between the two radix-16 passes goes through HALF a tile (16 rows x 8 columns) in two passes, in place
//     in the registers and without selects: lanes 8..15 of a unit run pass one on (-1)^n x[n] (the sign lives in their window
//     table), so their register j holds bin j ^ 8 (shift theorem) and "registers 0..7" are the diagonal blocks of the transpose for
//     every lane; what they receive sits in register n ^ 8, i.e. pass two sees its input rotated by 8 and its odd outputs negated
//     -- put right by eight packed multiplies with a per-lane +-1 (nfft 512), or by the same +-1 riding on the even / odd
//     recombination's operands (nfft 1024: no instruction of its own);
//   * the power spectrum reuses the tile's space, the item sums are compact, the log-mel block is [mel][16 frames] per wave with an
//     XOR swizzle (conflict-free for the log phase's column writes and the DCT's B-fragment reads without padding);
//   * the next round's samples are requested AFTER the real-FFT split (the FFT registers are dead by then), the DCT's A fragments
//     are fetched per chunk (L1 / L2 hits) instead of living in 48 registers.
// Results are bitwise those of frontend_pk.hip (same operations in the same order on every value; the first pass leaves out its adds of
// the FFT's zero padding, pk3_window_dft4 below, which moves the sign of zeros in front of the squares at most).
#include "frontend_plan.h"
#include "frontend_args.h"

namespace tcr {

// (v2 / v4, the packed-FP32 complex idioms c_*, row_swap, lane_gather, fast_log, pk_sq_pair: gfx950_isa.h)

namespace {

// One LDS read that the compiler does not pair with the next one.  Two 8-byte reads a few slots apart become one ds_read2_b64
// (two 4 x 16-lane accesses: 8 LDS-array cycles) where two ds_read_b64 (2 x 32 lanes each) take 2 + 2; the empty asm orders memory
// accesses, so neither the IR load vectoriser nor the DS load/store optimiser merges across it.  No instruction of its own (plain C++
// on the host emulator too); the compiler still counts the read on lgkmcnt and waits for it where the value is used.
template <class T> __device__ __forceinline__ T lds_read_unpaired(const T* p) {
    const T v = *p;
    asm volatile("" ::: "memory");
    return v;
}

// 4-point forward DFT (W4 = -i), in place: 8 packed instructions.
__device__ __forceinline__ void pk3_dft4(v2& a, v2& b, v2& c, v2& d) {
    const v2 t0 = a + c, t1 = a - c, t2 = b + d, t3 = b - d;
    a = t0 + t2;
    c = t0 - t2;
    b = c_submi(t1, t3);
    d = c_addmi(t1, t3);
}

// 16-point forward DFT in registers, natural order in and out (4 x 4 Cooley-Tukey) -- the operation order of frontend_pk.hip's:
// the four 4-point DFTs over n0 (pk3_dft16 below, or pk3_window_dft4 for the windowed first pass), then this.
__device__ __forceinline__ void pk3_dft16_tail(v2 (&v)[16]) {
    constexpr float C1 = 0.92387953251128673848f;   // cos(pi/8)
    constexpr float S1 = 0.38268343236508978178f;   // sin(pi/8)
    constexpr float R2 = 0.70710678118654752440f;   // sqrt(1/2)
    v[1 + 4] = c_mulk(v[1 + 4], (v2){C1, -S1});         // W^1
    v[1 + 8] = c_mulk(v[1 + 8], (v2){R2, -R2});         // W^2
    v[1 + 12] = c_mulk(v[1 + 12], (v2){S1, -C1});       // W^3
    v[2 + 4] = c_mulk(v[2 + 4], (v2){R2, -R2});         // W^2
    v[2 + 8] = c_submi((v2){0.f, 0.f}, v[2 + 8]);       // W^4 = -i
    v[2 + 12] = c_mulk(v[2 + 12], (v2){-R2, -R2});      // W^6
    v[3 + 4] = c_mulk(v[3 + 4], (v2){S1, -C1});         // W^3
    v[3 + 8] = c_mulk(v[3 + 8], (v2){-R2, -R2});        // W^6
    v[3 + 12] = c_mulk(v[3 + 12], (v2){-C1, S1});       // W^9
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1) pk3_dft4(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i + 1; j < 4; ++j) {
            const v2 t = v[4 * i + j];
            v[4 * i + j] = v[4 * j + i];
            v[4 * j + i] = t;
        }
}

__device__ __forceinline__ void pk3_dft16(v2 (&v)[16]) {
#pragma unroll
    for (int n0 = 0; n0 < 4; ++n0) pk3_dft4(v[n0], v[n0 + 4], v[n0 + 8], v[n0 + 12]);
    pk3_dft16_tail(v);
}

// The window multiply and the four 4-point DFTs of the FIRST radix-16 pass, for QV live inputs (x[q] w[q], q < QV; inputs QV .. 15
// are the zero padding of the FFT and are neither formed nor added).
// Which products fuse into the butterflies' first adds decides the bits, so it is spelled out and not left to the optimiser (whose
// choice moved when the adds around it changed): with t0 = a + c, t1 = a - c (t2, t3 from b, d likewise) the product of the FIRST
// operand (a = input n0, b = input n0 + 4) rides in the add as one fused multiply-add, the second operand's is rounded on its own.
// `fp contract(on)` forms exactly the fused multiply-adds that are written as one expression, and none across statements (the host
// emulator's target has no fused multiply-add, there the same expressions stay a multiply and an add, as they always were).
// A padded second operand: a + 0 and a - 0 are a, for every a but -0 (which a + 0 would turn into +0).  A zero's sign cannot reach an
// output: add, multiply and fused multiply-add of values that differ only in the sign of a zero differ at most in the sign of a zero,
// and the spectrum is squared (x x + y y is +0 for every zero x, y) before anything else reads it.
template <int QV>
__device__ __forceinline__ void pk3_window_dft4(const v2 (&x)[QV], const v2 (&w)[QV], v2 (&v)[16]) {
#pragma clang fp contract(on)
    static_assert(QV >= 8 && QV <= 16, "inputs n0 and n0 + 4 of every 4-point DFT are live");
#pragma unroll
    for (int n0 = 0; n0 < 4; ++n0) {
        v2 t0, t1, t2, t3;
        if (n0 + 8 < QV) {
            const v2 c = x[n0 + 8] * w[n0 + 8];
            t0 = x[n0] * w[n0] + c;
            t1 = x[n0] * w[n0] - c;
        } else {
            t0 = t1 = x[n0] * w[n0];
        }
        if (n0 + 12 < QV) {
            const v2 d = x[n0 + 12] * w[n0 + 12];
            t2 = x[n0 + 4] * w[n0 + 4] + d;
            t3 = x[n0 + 4] * w[n0 + 4] - d;
        } else {
            t2 = t3 = x[n0 + 4] * w[n0 + 4];
        }
        v[n0] = t0 + t2;
        v[n0 + 8] = t0 - t2;
        v[n0 + 4] = c_submi(t1, t3);
        v[n0 + 12] = c_addmi(t1, t3);
    }
}

__device__ __forceinline__ void pk3_real_pair_power(v2 zk, v2 zn, v2 wmi, float& p_lo, float& p_hi) {
    const v2 A = c_addc(zk, zn), D = c_subc(zk, zn);
    const v2 C = c_mul(D, wmi);
    pk_sq_pair(A, C, p_lo, p_hi);
}

// What an instance takes out of its round loop: per-round bookkeeping whose result is the same in every round of a chunk, or follows
// from the previous round's by an addition.  Each item holds registers through the round body (the compiler then hoists the masks,
// shifts, compares and LDS addresses made from a descriptor as well, which is most of the saving and most of the registers), so an
// instance takes an item only where it stays at three waves per SIMD without scratch it did not have; the table behind the choice
// is profiles/fe_carry_kernel_regs.txt, the counts are in OPTLOG.md "Front-end round bookkeeping".
constexpr int kPk3Carry = 1;        // frame coordinates stepped from round to round (frame_next) instead of worked out from the frame number
constexpr int kPk3BandsReg = 2;     // the bands' item ranges in registers for a chunk's rounds (else one LDS read per band and round)
constexpr int kPk3ItemsReg = 4;     // the trips' item descriptors likewise (else one LDS read per trip and round)
constexpr int pk3_round_policy(int nc, int qv) {
#ifdef TCR_PK3_POLICY
    return TCR_PK3_POLICY;          // (what-if builds: one policy for every instance, TCR_BUILD_EXTRA=-DTCR_PK3_POLICY=n)
#endif
    if (nc == 512) return qv == 10 ? kPk3BandsReg | kPk3ItemsReg : 0;   // 15 / 16 live inputs: at the 168-register ceiling as they are
    return qv == 16 ? kPk3ItemsReg : kPk3Carry | kPk3ItemsReg;           // nfft 512: four bands per lane, their hoisted unpacking spills
}

}  // namespace

// LDS of one workgroup (bytes): 4 waves x (tile / power 4608 + item sums FPWV x 832 + log-mel 4096) + slopes + items
//   nfft 1024: 18432 + 6656 + 16384 + 6144       = 47616      nfft 512: 18432 + 13312 + 16384 + 3072 + 768 = 51968
// three workgroups per CU: <= 54613.
// STREAM (stream.hip): the k = a.n_frames new frames of each stream of a streaming detector -- frame g is frame t = g % k of stream
// g / k, read from the stream's staging row (a.wav, row stride a.n_samples) at t * hop like an utterance's, and written to window
// column T - k + t of a window of a.tp = T + 2 kHalo columns; the halo zeroing keys on the window column.  Per-frame arithmetic
// unchanged, and the argument block is the same (the column offset is derived from tp), so the other instances compile as before.
template <int NC, int QV, bool MAG, bool STREAM>
__global__ __launch_bounds__(256, 3) void frontend_pk3_kernel(const FrontendArgs a) {
    constexpr int LPF = NC / 16;            // lanes per frame
    constexpr int FPR = 256 / LPF;          // frames per round (workgroup)
    constexpr int FPWV = FPR / 4;           // frames per round and wave
    constexpr int SUB = NC / 256;           // 256-point units per frame
    constexpr int NBINS = NC + 1;
    constexpr int NMEL = 64, NSEG = NMEL + 1;
    constexpr int RS = 9;                   // row of the 16 x 8 half tile (v2 units): odd -> the 16 lanes of a ds_write_b64 group hit 32 banks
    constexpr int UNITSZ = 16 * RS;         // half tile of one 256-point unit
    constexpr int TILEW = 4 * UNITSZ;       // v2 per wave (4 units)
    constexpr int PLD = NBINS + (LPF >= 32 ? 31 : 15);      // power-spectrum row stride (frontend_pk.hip)
    static_assert(FPWV * PLD <= 2 * TILEW, "the power spectrum of a wave's frames lives in its tile space");
    constexpr int kMelItemBins = mel_item_bins(NC);
    constexpr int kPolicy = pk3_round_policy(NC, QV);
    constexpr bool kCarry = kPolicy & kPk3Carry, kBandsReg = kPolicy & kPk3BandsReg, kItemsReg = kPolicy & kPk3ItemsReg;
    constexpr int NIT = mel_items_fast(NC);         // items of the unrolled trips; the launcher sends filterbanks with more to frontend_pk.hip
    constexpr int USZ = NIT + 8; static_assert(NIT + 3 <= USZ, "the log phase reads up to three cells from a band's first item");
                       // item sums of one frame (+ the cell of the empty slots, mel_dummy_item, + the log phase's read-ahead)
    static_assert(mel_dummy_item(NC, NIT) < USZ, "the empty slots' cell lies inside the item-sum row");
    constexpr int TRIPS = mel_trips(NC);

    __shared__ v2 s_t[4 * TILEW];
    __shared__ v2 s_ud[4 * FPWV * USZ];
    __shared__ float s_lm[4 * NMEL * 16];
    __shared__ v4 s_wit[kMelItemBins / 2 * NIT];    // [bin pair][item]: the slopes of bins 2 bp and 2 bp + 1 in one ds_read_b128
    __shared__ int s_items[NIT];            // the trips' item descriptors
    __shared__ int s_band[NMEL];            // the bands' item ranges: first item | first item of the next band << 8 | of the one after << 16
    __shared__ v2 s_wnd[QV * LPF];          // signed window [q][lane of the frame]: samples 2 (SUB (l + 16 q) + u), + 1

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const float fold = MAG ? 0.5f : 0.25f;
        const v2* wit = reinterpret_cast<const v2*>(a.mel_wit);
        for (int i = tid; i < kMelItemBins / 2 * NIT; i += 256) {
            const int bp = i / NIT, it = i % NIT;
            const v2 w0 = wit[2 * bp * NIT + it] * fold, w1 = wit[(2 * bp + 1) * NIT + it] * fold;
            s_wit[i] = (v4){w0.x, w0.y, w1.x, w1.y};
        }
        for (int i = tid; i < NIT; i += 256) s_items[i] = a.mel_items[i];
        if (tid < NMEL) s_band[tid] = a.mel_ifirst[tid] | (a.mel_ifirst[tid + 1] << 8) | (a.mel_ifirst[tid + 2] << 16);
        for (int i = tid; i < QV * LPF; i += 256) {
            const int q = i / LPF, lfi = i % LPF;
            s_wnd[i] = *reinterpret_cast<const v2*>(a.window_sgn + 2 * (SUB * ((lfi & 15) + 16 * q) + (lfi >> 4)));
        }
    }
    const v2* tw256 = reinterpret_cast<const v2*>(a.tw256);
    const v2* tw_real = reinterpret_cast<const v2*>(a.tw_real);
    const v2* tw_combine = reinterpret_cast<const v2*>(a.tw_combine);
    // round-invariant per-lane tables that stay in registers (64): the inter-pass twiddles (32), the real-FFT split's and the even /
    // odd recombination's (16 + 16).  The window (20 - 32 registers) does not: it is read from its LDS copy (s_wnd) every round, held
    // for the length of the window multiply, so that 3 waves per SIMD (<= 168 registers) hold without scratch.
    v2 tw[16], twr[8], twc[8];
    float sgn;
    {
        const int lf = tid % LPF, l = tid & 15, h = l >> 3;
        // the (-1)^h of the second pass's odd outputs.  nfft 1024: every odd output goes through the row swap into a lane of the frame's
        // second unit (same l, so same h) -- as its own odd register, or as the first unit's that it receives -- and the lanes of the
        // first unit keep and receive even registers only: the sign is applied there, behind the swap (s_fold below)
        sgn = h && (SUB == 1 || lf >= 16) ? -1.f : 1.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) tw[j] = tw256[l * 16 + (j ^ (8 * h))];    // lanes 8..15: register j holds bin j ^ 8 after the first pass
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = lf + LPF * i;
            const v2 w = tw_real[k];
            twr[i] = (v2){w.y, -w.x};           // -i W^k
            twc[i] = (SUB == 2) ? tw_combine[k] * sgn : (v2){1.f, 0.f};
        }
    }
    const v2 wm = tw_real[NC / 2];
    const v2 twmid = (v2){wm.y, -wm.x};

    const float inv_frames = 1.0f / (float)a.n_frames;
    const int rounds = a.rounds;            // <= 16 / FPWV; chosen by the launcher
    const int fpwv = rounds * FPWV;         // frames per chunk and wave (the columns of its DCT tile)
    const int fpw = 4 * fpwv;               // frames per chunk
    v2 xa[QV];
    // The samples of frame g = chunk * fpw + wave * fpwv + rr * FPWV + fw: utterance n = g / n_frames, frame t = g % n_frames, from
    // this lane's first sample on (fsrc; the QV loads sit at constant offsets behind it).  frame_at works the coordinates out from g;
    // frame_next (kCarry) steps those of the previous round by FPWV frames: within a chunk a lane's g goes up by exactly FPWV per
    // round, i.e. by FPWV / n_frames utterances and step_r = FPWV % n_frames frames with at most one wrap of t behind them
    // (step_r < n_frames), whatever n_frames is (the streaming instance at k = 1 wraps every round).  Integer and address work only.
    int ft = 0;
    const float* fsrc = a.wav;
    const int step_r = FPWV % a.n_frames;
    const ptrdiff_t step_src = (ptrdiff_t)(FPWV / a.n_frames) * a.n_samples + (ptrdiff_t)step_r * a.hop;
    const ptrdiff_t step_src_wrap = step_src + a.n_samples - (ptrdiff_t)a.n_frames * a.hop;
    auto frame_at = [&](int chunk, int rr) {
        const int tid = (int)threadIdx.x;
        const int lf = tid % LPF, u = lf >> 4, l = tid & 15, fw = (tid & 63) / LPF;
        int g = chunk * fpw + wave * fpwv + rr * FPWV + fw;
        g = min(g, a.total_frames - 1);
        int n = (int)(((float)g + 0.5f) * inv_frames);          // g / n_frames: float multiply + one-step fix-up
        n += (n + 1) * a.n_frames <= g ? 1 : (n * a.n_frames > g ? -1 : 0);
        ft = g - n * a.n_frames;
        fsrc = a.wav + (size_t)n * a.n_samples + (size_t)ft * a.hop + 2 * (SUB * l + u);
    };
    auto frame_next = [&]() {
        const unsigned t = (unsigned)(ft + step_r), tm = t - (unsigned)a.n_frames;      // (tm: t wrapped, or past 2^31 where t < n_frames)
        fsrc += tm < t ? step_src_wrap : step_src;
        ft = (int)min(t, tm);
    };
    auto load_frame = [&](v2 (&dst)[QV]) {
#pragma unroll
        for (int q = 0; q < QV; ++q) dst[q] = *reinterpret_cast<const v2*>(fsrc + 2 * SUB * 16 * q);        // (8-byte aligned: launcher)
    };
    const int nchunks = (a.total_frames + fpw - 1) / fpw;
    frame_at(blockIdx.x, 0);
    load_frame(xa);
    __syncthreads();                        // the slope table / item list staged above (the only workgroup barrier)
    // De-phasing: the twelve waves of a CU start together and do identical work, so they would stay in lock step -- all in their VALU
    // phases, then all queueing at the LDS.  A one-off delay of (workgroup generation * 4 + wave) * stagger * 64 cycles spreads them over a round.
    if (a.stagger > 0) {
        const int steps = (((int)blockIdx.x / a.stagger_div) * 4 + wave) * a.stagger;
        for (int i = 0; i < steps; ++i) __builtin_amdgcn_s_sleep(1);
    }

#pragma unroll 1
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    // lane geometry re-derived per chunk from an opaque zero: the address arithmetic of the unrolled round body must not be hoisted
    // out of the chunk loop (it would stay live through the DCT section)
    const int tid = (int)threadIdx.x + opaque_zero();
    const int lane = tid & 63;
    const int lf = tid % LPF, u = lf >> 4, l = tid & 15, h = l >> 3;
    const int fw = lane / LPF;              // frame of the wave in this round
    v2* T = s_t + wave * TILEW + (lane >> 4) * UNITSZ;
    float* Pw = reinterpret_cast<float*>(s_t + wave * TILEW);
    float* LM = s_lm + wave * (NMEL * 16);
    // Round-invariant descriptors of this lane, per instance (pk3_round_policy) in registers for the length of a chunk's rounds -- read
    // here, from the opaque lane geometry, so that they are dead in the DCT section -- or re-read from LDS in every round.
    int item_d[kItemsReg ? TRIPS : 1], band_i[kBandsReg ? NMEL / LPF : 1];
    if (kItemsReg) {
#pragma unroll
        for (int tr = 0; tr < TRIPS; ++tr) item_d[kItemsReg ? tr : 0] = s_items[lf + LPF * tr];
    }
    if (kBandsReg) {
#pragma unroll
        for (int i = 0; i < NMEL / LPF; ++i) band_i[kBandsReg ? i : 0] = s_band[lf + LPF * i];
    }
#pragma unroll 1
    for (int r = 0; r < rounds; ++r) {
        // ---------------- window + first radix-16 pass ----------------
        // The window comes from LDS every round (20 registers for a moment instead of for the kernel's life; lanes 8..15 of a unit:
        // x[n] (-1)^n -- a.window_sgn carries the sign -- so that their register j holds bin j ^ 8 after the pass).
        v2 v[16];
        {
            const v2* wsrc = s_wnd + lf;
            v2 wnd[QV];
#pragma unroll
            for (int q = 0; q < QV; ++q) wnd[q] = lds_read_unpaired(wsrc + q * LPF);     // (ds_read_b64 each)
            pk3_window_dft4<QV>(xa, wnd, v);
        }
        pk3_dft16_tail(v);                                      // register j: bin j ^ 8h of this lane's 16 samples
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = c_mul(v[j], tw[j]);
        // ---------------- transpose through half a tile, two passes (diagonal blocks, then off-diagonal blocks) ----------------
        {
            v2* wa = T + (8 * h) * RS + (l & 7);
            v2* wb = T + (8 * (1 - h)) * RS + (l & 7);
            const v2* rd = T + l * RS;
#pragma unroll
            for (int j = 0; j < 8; ++j) wa[j * RS] = v[j];
            wave_sync();
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = lds_read_unpaired(rd + c);           // (RS odd: 32 distinct 8-byte slots per 32 lanes)
            wave_sync();
#pragma unroll
            for (int j = 0; j < 8; ++j) wb[j * RS] = v[8 + j];
            wave_sync();
#pragma unroll
            for (int c = 0; c < 8; ++c) v[8 + c] = lds_read_unpaired(rd + c);
        }
        // ---------------- second radix-16 pass: register n holds input n ^ 8h -> odd outputs carry (-1)^h ----------------
        pk3_dft16(v);
        const v2 s2 = (v2){sgn, sgn};
        if (SUB == 1) {
#pragma unroll
            for (int k1 = 1; k1 < 16; k1 += 2) v[k1] = v[k1] * s2;
        }
        wave_sync();                                            // (the tile space becomes the power spectrum)
        // ---------------- real-FFT split -> 4 x power spectrum (frontend_pk.hip) ----------------
        {
            float* P = Pw + fw * PLD;
            const int partner = (lane & ~(LPF - 1)) | (SUB == 2 ? (l ? (16 * (1 - u) + 16 - l) : 16 * u) : ((16 - l) & 15));
            if (SUB == 2) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float ex = v[2 * i].x, ey = v[2 * i].y, ox = v[2 * i + 1].x, oy = v[2 * i + 1].y;
                    row_swap(ex, ox, lane);
                    row_swap(ey, oy, lane);
                    // s_fold: with s = this lane's sign, Z = s e +- (s o) w.  The sign rides on the operations that read e and o instead of
                    // eight multiplies in front of them: o (s w) negates the same inputs of the same multiply / fused multiply-adds as
                    // (s o) w, and fma(e, s, +-t) rounds s e +- t once, s e being exact -- the same value, zeros' signs included.
                    const v2 t = c_mul((v2){ox, oy}, twc[i]);   // (twc carries s)
                    const v2 e = (v2){ex, ey};
                    v[2 * i] = __builtin_elementwise_fma(e, s2, t);         // Z[k_i]
                    v[2 * i + 1] = __builtin_elementwise_fma(e, s2, -t);    // Z[k_i + 256]
                }
            }
            // Bins k_i = lf + LPF i and NC - k_i of a lane are LPF floats apart from one i to the next: two bins of the lower half, then
            // two of the upper half, go out next to each other, so that each pair is ONE two-address store (ds_write2_b32: one address
            // register and one issue for two dwords) -- the lower / upper stores of one i alternate bases the compiler cannot tell apart.
            float* Plo = P + lf;                            // bin lf + LPF i at + LPF i
            float* Phi = P + (NC - LPF * 7 - lf);           // bin NC - lf - LPF i at + LPF (7 - i)
            v2 prev = v[0];
#pragma unroll
            for (int i2 = 0; i2 < 8; i2 += 2) {
                float plo[2], phi[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int i = i2 + j;                   // bin k = lf + LPF i: 0 .. NC/2-1
                    const v2 zk = SUB == 2 ? v[2 * i] : v[i];
                    const v2 src = SUB == 2 ? v[15 - 2 * i] : v[15 - i];
                    const v2 g = (v2){lane_gather(src.x, partner), lane_gather(src.y, partner)};
                    const v2 zn = lf == 0 ? prev : g;
                    prev = g;
                    pk3_real_pair_power(zk, zn, twr[i], plo[j], phi[j]);
                    if (MAG) { plo[j] = sqrtf(plo[j]); phi[j] = sqrtf(phi[j]); }
                }
                Plo[LPF * i2] = plo[0];
                Plo[LPF * (i2 + 1)] = plo[1];
                Phi[LPF * (7 - i2)] = phi[0];
                Phi[LPF * (6 - i2)] = phi[1];
            }
            if (lf == 0) {                                  // the self-paired middle bin k = NC/2
                const v2 z = SUB == 2 ? v[1] : v[8];
                float plo, phi;
                pk3_real_pair_power(z, z, twmid, plo, phi);
                if (MAG) plo = sqrtf(plo);
                P[NC / 2] = plo;
            }
            if (lf < PLD - NBINS) P[NBINS + lf] = 0.f;      // row pad: read (times a zero slope) past an item's end; the space held tile data
        }
        // ---------------- the next round's samples (the FFT registers are free) ----------------
        // (a chunk's first round, and every round of a chunk that reaches past the last frame -- the clamp --, from g)
        {
            const bool jump = r + 1 == rounds;
            const int ch = jump ? chunk + (int)gridDim.x : chunk;
            if (ch < nchunks) {
                if (kCarry && !jump && (ch + 1) * fpw <= a.total_frames) frame_next();
                else frame_at(ch, jump ? 0 : r + 1);
                load_frame(xa);
            }
        }
        wave_sync();
        // ---------------- sparse mel: one item (<= 8 bins of one segment) per lane and trip, one packed FMA per bin ----------------
        v2* UD = s_ud + (wave * FPWV + fw) * USZ;
        int bi_pre[NMEL / LPF];                             // the bands' item ranges: requested with the trips' operands, used by the log phase
#pragma unroll
        for (int i = 0; i < NMEL / LPF; ++i) bi_pre[i] = kBandsReg ? band_i[kBandsReg ? i : 0] : s_band[lf + LPF * i];
        {
            const float* P = Pw + fw * PLD;
#pragma unroll
            for (int tr = 0; tr < TRIPS; ++tr) {            // (unrolled: the trips' descriptor and operand reads overlap instead of TRIPS dependent LDS round trips in a row)
                const int it = lf + LPF * tr;
                const int d = kItemsReg ? item_d[kItemsReg ? tr : 0] : s_items[it];     // (tr: a constant of the unrolled trip)
                const float* pk = P + (d & 1023);
                const v4* wk = s_wit + it;
                float p[kMelItemBins];
                v2 wv[kMelItemBins];
#pragma unroll
                for (int b = 0; b < kMelItemBins; ++b) p[b] = pk[b];
#pragma unroll
                for (int bp = 0; bp < kMelItemBins / 2; ++bp) {    // (ds_read_b128, 16 consecutive lanes on 256 consecutive bytes: 4 cycles, no conflicts)
                    const v4 w = wk[bp * NIT];
                    wv[2 * bp] = (v2){w.x, w.y};
                    wv[2 * bp + 1] = (v2){w.z, w.w};
                }
                v2 ud = (v2){0.f, 0.f};
#pragma unroll
                for (int b = 0; b < kMelItemBins; ++b) ud = __builtin_elementwise_fma(wv[b], (v2){p[b], p[b]}, ud);
                UD[(d >> 21) & 255] = ud;                    // (the slot's LOGICAL item; empty slots: mel_dummy_item)
            }
        }
        wave_sync();
        // ---------------- log(mel + 1e-6) -> [mel][frame ^ swizzle] ----------------
        {
            const int c = r * FPWV + fw;                    // column of the wave's DCT tile
            constexpr int NB = NMEL / LPF;
            constexpr int MAXC = NC == 512 ? 3 : 2;
            float up[NB][MAXC], dn[NB][MAXC];
#pragma unroll
            for (int i = 0; i < NB; ++i) {                  // every band's cells first (single ds_read_b64 each), the sums behind them
                const int bi = bi_pre[i];
                const int i0 = bi & 255, i1 = (bi >> 8) & 255;
#pragma unroll
                for (int cc = 0; cc < MAXC; ++cc) {
                    up[i][cc] = lds_read_unpaired(UD + i0 + cc).x;      // (i0, i1 <= NIT: inside the row; cells past the band's items are read and dropped)
                    dn[i][cc] = lds_read_unpaired(UD + i1 + cc).y;
                }
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int m = lf + LPF * i;
                const int bi = bi_pre[i];
                const int i0 = bi & 255, i1 = (bi >> 8) & 255, i2 = bi >> 16;
                // (nfft 1024: a segment has <= MAXC items -- the launcher sends other filterbanks to frontend_pk.hip --, so no loop behind
                //  the unconditional reads; nfft 512: the reference filterbank has a few 3-item segments, the loops stay)
                float mel = 0.f;
#pragma unroll
                for (int cc = 0; cc < MAXC; ++cc) mel += i0 + cc < i1 ? up[i][cc] : 0.f;
                if (NC != 512) for (int it = i0 + MAXC; it < i1; ++it) mel += UD[it].x;
#pragma unroll
                for (int cc = 0; cc < MAXC; ++cc) mel += i1 + cc < i2 ? dn[i][cc] : 0.f;
                if (NC != 512) for (int it = i1 + MAXC; it < i2; ++it) mel += UD[it].y;
                LM[m * 16 + (c ^ ((m >> 1) & 15))] = fast_log(a.log_floor ? fmaxf(mel, 1e-12f) : mel + 1e-6f);
            }
        }
        // (no sync: the next LDS phase that touches the item sums or the power spectrum sits behind the next round's syncs)
    }
    wave_sync();

    // ---------------- DCT-II on the matrix cores: a wave's own <= 16 frames, all coefficient tiles ----------------
    {
        const int kq = lane >> 4, col = lane & 15;
        const int g = chunk * fpw + wave * fpwv + col;
        const bool valid = col < fpwv && g < a.total_frames;
        const int gg = valid ? g : a.total_frames - 1;
        const int n = gg / a.n_frames;
        const int t = gg - n * a.n_frames;
        const int col0 = STREAM ? a.tp - 2 * kHalo - a.n_frames : 0;       // window column of the stream's first new frame (halo: column 0
                                                                            // is new only when k == T)
        float* dst = a.out + (size_t)n * a.n_coef * a.tp + kHalo + col0 + t;
        if (a.no_dct) {
            for (int m = kq; m < a.n_coef; m += 4) {
                if (valid) {
                    float* row = dst + (size_t)m * a.tp;
                    row[0] = LM[m * 16 + (col ^ ((m >> 1) & 15))];
                    if (t == 0 && (!STREAM || col0 == 0)) { row[-4] = 0.f; row[-3] = 0.f; row[-2] = 0.f; row[-1] = 0.f; }
                    if (t == a.n_frames - 1) { row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; row[4] = 0.f; }
                }
            }
        } else {
            constexpr int CT = NMEL / 16;                                   // coefficient tiles (n_coef <= NMEL)
            const int ntile = (a.n_coef + 15) >> 4;
            const int c0 = col ^ (kq >> 1);                                 // m = 4 st + kq: (m >> 1) & 15 = (2 st & 14) | (kq >> 1)
            float bv[NMEL / 4];
#pragma unroll
            for (int st = 0; st < NMEL / 4; ++st) bv[st] = LM[(4 * st + kq) * 16 + (c0 ^ ((2 * st) & 14))];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                if (ct < ntile) {                                           // (wave-uniform)
                    float av[NMEL / 4];
#pragma unroll
                    for (int st = 0; st < NMEL / 4; ++st) av[st] = a.dct_tab[(ct * (NMEL / 4) + st) * 64 + lane];
                    v4 acc = (v4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int st = 0; st < NMEL / 4; ++st) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st], bv[st], acc, 0, 0, 0);
                    if (valid) {
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {
                            const int c = 16 * ct + 4 * kq + rr;
                            if (c < a.n_coef) {
                                float* row = dst + (size_t)c * a.tp;
                                row[0] = acc[rr];
                                if (t == 0 && (!STREAM || col0 == 0)) { row[-4] = 0.f; row[-3] = 0.f; row[-2] = 0.f; row[-1] = 0.f; }
                                if (t == a.n_frames - 1) { row[1] = 0.f; row[2] = 0.f; row[3] = 0.f; row[4] = 0.f; }
                            }
                        }
                    }
                }
            }
        }
    }
    // (no barrier: the next chunk's first write to the log-mel block sits behind that chunk's wave-local syncs)
    }
}

// the launcher's own tests below, for a caller that needs to know before it launches (stream.hip refuses what pk3 would decline)
int frontend_pk3_supports(int nc, int win, int n_items) {
    const int sub = nc / 256;
    if ((nc != 256 && nc != 512) || (win & 1) || (win / 2) % (16 * sub) != 0) return 0;
    if (n_items < 0 || n_items > mel_items_fast(nc)) return 0;
    const int qv = win / (32 * sub);
    return (qv == 10 || qv == 15 || qv == 16) ? 1 : 0;     // the instances of TCR_FPK3 below
}

// returns 1 (nothing launched) when the configuration needs another kernel: unaligned frames, a window whose valid radix-16 inputs
// differ from lane to lane, or a filterbank with more items than the unrolled trips take / with a segment of more items than the log
// phase reads (n_items < 0: frontend_mel_item_count)
template <bool STREAM>
static int launch_pk3(int nc, const FrontendArgs& a0, int n_items, hipStream_t s) {
    const int sub = nc / 256;
    if (!a0.aligned || (a0.win & 1) || (a0.win / 2) % (16 * sub) != 0) return 1;
    if (a0.total_frames >= (1 << 23)) return 1;                // (the frame -> utterance split uses a float reciprocal)
    if (n_items < 0 || n_items > mel_items_fast(nc)) return 1;
    const int qv = a0.win / (32 * sub);
    // Persistent workgroups (3 per CU) walk chunks of rounds x (4096 / nc) frames: at most 16 frames per wave (one DCT tile).  The cost
    // model of frontend_pk.hip's launcher with three slots per CU (a chunk costs rounds + ~1.45 rounds).
    FrontendArgs a = a0;
    int grid = 0;
    {
        const int fpr = 4096 / nc, max_rounds = 64 / fpr, slots = 3 * device_cus();
        int best = max_rounds;
        float best_cost = 3.4e38f;
        const int r_min = ceil_div(a.total_frames, fpr) <= slots / 2 ? 1 : (max_rounds + 1) / 2;
        for (int r = max_rounds; r >= r_min; --r) {
            const int chunks = ceil_div(a.total_frames, r * fpr);
            const int full = chunks / slots, rest = chunks % slots;
            const float gens = (float)full + (rest == 0 ? 0.f : (3 * rest <= slots ? 0.45f : (3 * rest <= 2 * slots ? 0.75f : 1.f)));
            const float cost = gens * ((float)r + 1.45f);
            if (cost < best_cost * 0.995f) { best_cost = cost; best = r; }
        }
        const int knob = tune_get(TCR_TUNE_FRONTEND);
        if (knob >= 10 && knob < 30) best = min(max(knob - 10, 1), max_rounds);
        if (a0.rounds > 0) best = min(a0.rounds, max_rounds);      // (tcr_frontend_fwd_rounds: the caller's per-call choice)
        a.rounds = best;
        grid = min(ceil_div(a.total_frames, best * fpr), slots);
        const int cap = tune_get(TCR_TUNE_FE_GRID);
        if (cap > 0) grid = min(grid, cap);
        a.stagger = tune_get(TCR_TUNE_FE_STAGGER);
        a.stagger_div = device_cus();
    }
#define TCR_FPK3(NC_, QV_)                                                                                          \
    if (nc == NC_ && qv == QV_) {                                                                                   \
        if (a.magnitude) hipLaunchKernelGGL((frontend_pk3_kernel<NC_, QV_, true, STREAM>), dim3(grid), dim3(256), 0, s, a); \
        else hipLaunchKernelGGL((frontend_pk3_kernel<NC_, QV_, false, STREAM>), dim3(grid), dim3(256), 0, s, a);            \
        return check_launch("frontend_pk3_kernel");                                                                 \
    }
    TCR_FPK3(512, 10)   // 40 ms window @ 16 kHz, FFT 1024
    TCR_FPK3(256, 15)   // 30 ms window, FFT 512
    TCR_FPK3(512, 16)
    TCR_FPK3(256, 16)
    TCR_FPK3(256, 10)   // 20 ms window, FFT 512
    TCR_FPK3(512, 15)
#undef TCR_FPK3
    return 1;
}

int launch_frontend_pk3(int nc, const FrontendArgs& a, int n_items, hipStream_t s) { return launch_pk3<false>(nc, a, n_items, s); }
int launch_frontend_pk3_stream(int nc, const FrontendArgs& a, int n_items, hipStream_t s) { return launch_pk3<true>(nc, a, n_items, s); }

}  // namespace tcr

// The streaming detector (tcr_stream_*) and the many-step calls (tcr_scan, tcr_stream_scan) that drive the STREAM instances are
// compiled in this translation unit, and the detection sweep over a scan's outputs (tcr_detect_sweep) next to the scan.
#include "stream.hip"
#include "scan.hip"
#include "sweep.hip"
#include "detect_grid.hip"
#include "scan_select.hip"
#include "mine.hip"
#include "compose.hip"
#include "phrase.hip"
#include "capture.hip"
#include "resample.hip"
#include "stream_cascade.hip"
#include "dtw.hip"
#include "reverb.hip"
