// Reverberation on the device (tcr_reverb): every clip of a table convolved with its room impulse response out of a bank, int16 pools
// or float32 recordings in, packed float32 and / or int16 out.  One launch for the whole table, one-second clips and a ten-minute
// recording alike: the work is the tiles of TCR_REVERB_TILE outputs, a workgroup finds its clip by one binary search of tile_off.
//
// The rule (include/tcresnet_hip.h): output i of a clip of n samples under a response of L taps is the fmaf chain from 0.f over the
// input index jj ascending, acc = fmaf(h[i - jj], x[jj], acc), jj = max(0, i - L + 1) .. min(i, n - 1).  That is the k-ordered chain of
// v_mfma_f32_16x16x4_f32, so the hot loop is the exact-f32 matrix core on a banded Toeplitz product.  For a block of 256 outputs
// i = i0 + 16 b + a (a the row, b the column):
//     Y[a][b] = sum_k H[a][k] X[k][b],   H[a][k] = h[a + L - 1 - k] (0 outside 0 .. L - 1),   X[k][b] = x[i0 - (L - 1) + 16 b + k]
// k = 0 .. L + 14 ascending is the input index ascending for every output; a term whose h or x is a padding zero is fmaf(0, finite,
// acc) and leaves acc's bits alone, so neither the tile, the stage grid nor what is skipped shows in a sample.
//
// A workgroup is four waves; a wave owns kRvBlocks = 4 column blocks (1024 consecutive outputs) in 16 accumulator registers, so
// one H fragment feeds four MFMAs.  The k loop runs in stages of TCR_REVERB_STAGE: per stage the workgroup stages
//   s_x: the TILE + STAGE - 16 input samples x[t0 - (L - 1) + ks ..] the tile's columns read, decoded to float32, zeros outside
//        0 .. n - 1, at a pitch of 18 words per 16 samples -- the B operand reads sample 16 b + k, a stride of 16 words, which a
//        32-lane half of ds_read_b32 would serve 8-way conflicted; 18 b (mod 32) runs through the sixteen even banks once, and the
//        half's second k through the odd ones;
//   s_h: the STAGE + 15 taps h[L - ks - STAGE ..] in their own order (lane (a, k) reads word a + STAGE - 1 - k: a half's 32 lanes
//        read 17 consecutive words, equal addresses broadcast), zeros outside 0 .. L - 1.
// The accumulators stay in registers across the stages.  Skipped, each bit-neutral: a stage whose staged span misses 0 .. n - 1
// (the whole workgroup, so the barriers stay uniform), within a stage the 16-k groups whose samples miss it for all of the wave's
// columns, and a wave whose outputs lie beyond the clip's m.  The cost is about outputs x min(L, n + tile), not outputs x L.
//
// Memory: every global load is one element, its index checked against the clip (0 .. n - 1, 0 .. L - 1) AND against the buffer
// (in_samples, ir_floats), so nothing outside either buffer is touched whatever the tables hold.  A lane holds four consecutive
// outputs; it stores them as one 16-byte (int16: 8-byte) word only where all four are the clip's own and the address is aligned,
// element by element otherwise: out_off is arbitrary, and a wide store across a clip's end would race with the neighbour's workgroup.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after mine.hip, whose int16 rounding it shares).
#pragma once
#include <algorithm>

namespace tcr {

namespace {

constexpr int kRvTile = TCR_REVERB_TILE;
constexpr int kRvStage = TCR_REVERB_STAGE;
constexpr int kRvThreads = 256;
constexpr int kRvBlocks = 4;                            // column blocks (256 outputs each) per wave
constexpr int kRvWaveOut = 256 * kRvBlocks;             // outputs per wave
static_assert(kRvTile == kRvWaveOut * (kRvThreads / 64), "reverb_kernel: four waves of four 16 x 16 column blocks");
static_assert(kRvStage % 16 == 0 && kRvStage >= 16, "reverb_kernel: a stage is whole groups of 16 k");
constexpr int kRvSpan = kRvTile + kRvStage - 16;        // staged input samples per stage
constexpr int kRvPitch = 18;                            // LDS words per 16 staged samples
constexpr int kRvXWords = kRvSpan / 16 * kRvPitch;
constexpr int kRvHWords = kRvStage + 15;

}  // namespace

struct ReverbArgs {
    const void* in;
    const int64_t* in_off;      // [n_clips]
    const int64_t* in_len;
    const float* ir;
    const int64_t* ir_off;      // per response
    const int32_t* ir_len;
    const int32_t* clip_ir;     // [n_clips]
    const int64_t* out_off;     // [n_clips + 1]
    const int64_t* tile_off;    // [n_clips + 1]
    float* out;                 // packed, or null
    int16_t* out_pcm;
    int64_t in_samples, ir_floats;
    int n_clips, in_format;
};

__global__ __launch_bounds__(kRvThreads) void reverb_kernel(const ReverbArgs a) {
    __shared__ float s_x[kRvXWords];
    __shared__ float s_h[kRvHWords];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);    // (uniform: the k loop's bounds are scalars)
    // the clip of this tile and what is wave-uniform about it (scalar loads)
    const int64_t tile = blockIdx.x;
    const int j = ragged_signal(a.tile_off, a.n_clips, tile);
    const int64_t o0 = a.out_off[j];
    const int64_t m = a.out_off[j + 1] - o0;
    const int64_t t0 = (tile - a.tile_off[j]) * kRvTile;                // the tile's first output, counted within the clip
    if (t0 < 0 || t0 >= m) return;                                      // (a table that does not match out_off: nothing to write)
    const int mt = (int)std::min<int64_t>(kRvTile, m - t0);
    const int64_t n = std::max<int64_t>(a.in_len[j], 0), x0 = a.in_off[j];
    const int r = a.clip_ir[j];
    const int L = std::min(std::max(a.ir_len[r], 0), TCR_REVERB_TAPS_MAX);
    const int64_t h0 = a.ir_off[r];
    const int w0 = wave * kRvWaveOut;                                   // the wave's first output within the tile
    const bool live = w0 < mt;
    v4 acc[kRvBlocks];
#pragma unroll
    for (int c = 0; c < kRvBlocks; ++c) acc[c] = (v4){0.f, 0.f, 0.f, 0.f};
    const int stages = (L + 15 + kRvStage - 1) / kRvStage;
    for (int s = 0; s < stages; ++s) {
        const int ks = s * kRvStage;
        const int64_t xb = t0 - (L - 1) + ks;                           // the input index of staged sample 0
        if (xb >= n || xb + kRvSpan <= 0) continue;                     // the whole span is padding (uniform over the workgroup)
        __syncthreads();                                                // (the stage before has been read)
        for (int e = tid; e < kRvSpan; e += kRvThreads) {
            const int64_t i = xb + e, at = x0 + i;
            float v = 0.f;
            if (i >= 0 && i < n && at >= 0 && at < a.in_samples)
                v = a.in_format ? (float)static_cast<const int16_t*>(a.in)[at] * (1.0f / 32768.0f) : static_cast<const float*>(a.in)[at];
            s_x[(e >> 4) * kRvPitch + (e & 15)] = v;
        }
        const int hb = L - ks - kRvStage;                               // the tap index of s_h[0]
        for (int e = tid; e < kRvHWords; e += kRvThreads) {
            const int i = hb + e;
            const int64_t at = h0 + i;
            s_h[e] = (i >= 0 && i < L && at >= 0 && at < a.ir_floats) ? a.ir[at] : 0.f;
        }
        __syncthreads();
        if (!live) continue;
        // the wave's column c (0 .. 63) reads input xw + 16 c + k at stage position k: the 16-k groups that can reach 0 .. n - 1
        const int64_t xw = xb + w0;
        const int k_lo = (int)std::min<int64_t>(std::max<int64_t>(-xw - 16 * (16 * kRvBlocks - 1), 0), kRvStage) & ~15;
        const int k_hi = (int)std::min<int64_t>(std::max<int64_t>(n - xw, 0), kRvStage);
        const float* xp = s_x + kRvPitch * ((w0 >> 4) + (lane & 15) + (k_lo >> 4)) + (lane >> 4);
        const float* hp = s_h + (lane & 15) + kRvStage - 1 - k_lo - (lane >> 4);
        for (int kk = k_lo; kk < k_hi; kk += 16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float hv = hp[-4 * q];
#pragma unroll
                for (int c = 0; c < kRvBlocks; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv, xp[c * 16 * kRvPitch + 4 * q], acc[c], 0, 0, 0);
            }
            xp += kRvPitch;
            hp -= 16;
        }
    }
    if (!live) return;
    // lane (col b = lane & 15, rows 4 (lane >> 4) + 0 .. 3) of block c holds outputs w0 + 256 c + 16 b + 4 (lane >> 4) + 0 .. 3
#pragma unroll
    for (int c = 0; c < kRvBlocks; ++c) {
        const int d = w0 + 256 * c + 16 * (lane & 15) + 4 * (lane >> 4);
        if (d >= mt) continue;
        const int64_t p = o0 + t0 + d;
        const int cnt = std::min(4, mt - d);
        if (a.out) {
            float* q = a.out + p;
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(q) & 15) == 0) mine_store4(q, acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
            else
                for (int k = 0; k < cnt; ++k) q[k] = acc[c][k];
        }
        if (a.out_pcm) {
            int16_t* q = a.out_pcm + p;
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(q) & 7) == 0) mine_store4(q, acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
            else
                for (int k = 0; k < cnt; ++k) q[k] = mine_pcm(acc[c][k]);
        }
    }
}

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_reverb(int64_t n_clips, const void* in, int in_format, int64_t in_samples, const int64_t* in_off, const int64_t* in_len,
                          const float* ir, int64_t ir_floats, const int64_t* ir_off, const int32_t* ir_len, const int32_t* clip_ir,
                          const int64_t* out_off, const int64_t* tile_off, int64_t total_tiles, float* out, int16_t* out_pcm,
                          void* stream) {
    const char* what = "tcr_reverb";
    TCR_REQUIRE(out || out_pcm, "%s: out and out_pcm are both null", what);
    TCR_REQUIRE(n_clips >= 0, "%s: n_clips must be >= 0 (got %lld)", what, (long long)n_clips);
    TCR_REQUIRE(in_format == 0 || in_format == 1, "%s: unknown in_format %d (0 float32, 1 int16)", what, in_format);
    TCR_REQUIRE(total_tiles >= 0 && in_samples >= 0 && ir_floats >= 0, "%s: negative count (total_tiles %lld, in_samples %lld, ir_floats %lld)",
                what, (long long)total_tiles, (long long)in_samples, (long long)ir_floats);
    TCR_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: out must be 4-byte aligned", what);
    TCR_REQUIRE((reinterpret_cast<uintptr_t>(out_pcm) & 1) == 0, "%s: out_pcm must be 2-byte aligned", what);
    TCR_REQUIRE((reinterpret_cast<uintptr_t>(ir) & 3) == 0, "%s: ir must be 4-byte aligned", what);
    TCR_REQUIRE((reinterpret_cast<uintptr_t>(in) & (in_format ? 1 : 3)) == 0, "%s: in must be aligned to its elements", what);
    if (n_clips == 0) return TCR_OK;
    TCR_REQUIRE(in && in_off && in_len && ir && ir_off && ir_len && clip_ir && out_off && tile_off, "%s: null argument", what);
    if (total_tiles == 0) return TCR_OK;
    TCR_REQUIRE(n_clips < ((int64_t)1 << 31), "%s: %lld clips are too many for one launch", what, (long long)n_clips);
    TCR_REQUIRE(total_tiles < ((int64_t)1 << 31), "%s: %lld tiles are too many for one launch", what, (long long)total_tiles);
    ReverbArgs a{};
    a.in = in; a.in_off = in_off; a.in_len = in_len; a.ir = ir; a.ir_off = ir_off; a.ir_len = ir_len; a.clip_ir = clip_ir;
    a.out_off = out_off; a.tile_off = tile_off; a.out = out; a.out_pcm = out_pcm; a.in_samples = in_samples; a.ir_floats = ir_floats;
    a.n_clips = (int)n_clips; a.in_format = in_format;
    hipLaunchKernelGGL(reverb_kernel, dim3((unsigned)total_tiles), dim3(kRvThreads), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("reverb_kernel");
}
