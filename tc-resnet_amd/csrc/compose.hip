// Composing labelled test recordings on the device (tcr_compose, tcr_pcm_energy): dataset clips pasted at known times onto looping
// background noise, N recordings of different lengths written straight into the packed layout tcr_scan_ragged takes, from the int16
// pools the training input stage holds.
//
// tcr_compose: the PACKED samples are cut into tiles of TCR_COMPOSE_TILE and a workgroup composes kComposeRun consecutive ones, so the
// work is the packed total whatever the recordings' lengths, and -- the packed base being aligned and the tile a multiple of four -- every store but the total's last is a
// 16-byte one (int16: 8-byte) whatever the recording's offset.  Everything about the tile is wave-uniform and comes through scalar
// loads: the recordings it touches (one binary search of sample_offsets, then the table in order), per recording the first placement
// that can reach the tile (one binary search over the placements' ends, which are non-decreasing because the placements are sorted
// and disjoint) and the background phase at the tile's first sample (the one 64-bit modulo per tile and recording); the tiles behind a workgroup's
// first step on from where the one before stopped instead of searching (measured: OPTLOG.md "Composing").  The lanes then
// walk the few placements that intersect the tile, each taking the samples it covers, and find their background sample by one
// compare against the wrap point (background recordings of at least a tile) or a 32-bit modulo (shorter ones).  The arithmetic is
// augment.hip's, operation for operation: two multiplies for the foreground (the first exact), one multiply and one add, never an
// fma, for the mix, the clip.  2-byte loads, as there: clip_off, place_first and the background phase are arbitrary, and augment.hip
// measured a thread's eight independent 2-byte loads feeding two 16-byte stores above lane-contiguous loads with narrow stores.
//
// tcr_pcm_energy: exact integer sums of squares.  A clip is cut at its 16-byte-aligned elements into groups of kEnergyGroup 16-byte
// loads (eight samples each); workgroup j sums clip j's first group and its unaligned ends, and behind those n workgroups come
// kEnergyParts helpers per 64 clips that share out the further groups of the long ones (a minute of background is 59 groups), so
// no workgroup walks a long recording alone and a pool of one-second clips pays one idle workgroup per four clips.  Every group's
// sum goes into the zeroed table with one 64-bit integer add: integer sums, so neither the order nor the launch shape shows.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after mine.hip, whose int16 rounding it shares).
#pragma once
#include <algorithm>

namespace tcr {

namespace {

constexpr int kComposeTile = TCR_COMPOSE_TILE;
static_assert(kComposeTile == 2048, "compose_kernel: 256 threads x two quads of four samples");
constexpr int kComposeRun = 4;                          // tiles a workgroup composes one after the other
constexpr int kEnergyGroup = 2048;                      // 16-byte loads per group: 256 threads x 8
constexpr int kEnergyParts = 16;                        // helper workgroups per 64 clips

}  // namespace

struct ComposeArgs {
    const int64_t* sample_off;  // [N + 1]
    const int16_t* pcm;
    const int32_t* place_off;   // [N + 1]
    const int64_t* place_clip_off;
    const int32_t* place_len;
    const int64_t* place_first;
    const float* place_gain;
    const int16_t* bg;
    const int64_t* bg_off;      // [N]
    const int64_t* bg_len;
    const int64_t* bg_phase;
    const float* bg_vol;        // [N] or null
    float* out;                 // packed, or null
    int16_t* out_pcm;
    int64_t total;
    int N, run;                 // run: tiles per workgroup
};

// clip(bg / 32768 * vol + fg, -1, 1): tf.multiply then tf.add, two roundings (augment_kernel's mix)
__device__ __forceinline__ float compose_mix(float bgv, float vol, float fg) {
#pragma clang fp contract(off)
    const float scaled = bgv * vol;
    const float o = scaled + fg;
    return fminf(fmaxf(o, -1.0f), 1.0f);
}

// A workgroup composes a.run consecutive tiles.  Thread t produces a tile's samples 4 t .. 4 t + 3 and 1024 + 4 t .. 1024 + 4 t + 3.
// Positions inside a tile are ints; what is 64-bit (packed and pool positions) is wave-uniform.  The first tile finds its recording
// and each recording's first placement by binary search; the tiles behind it start from where the one before stopped (n_at: its
// first recording; of recording j_rec the placement j_at, the last one that began in front of that tile's end) and step forward.
__global__ __launch_bounds__(256) void compose_kernel(const ComposeArgs a) {
    const int64_t tiles = (a.total + kComposeTile - 1) / kComposeTile;
    const int64_t tile0 = (int64_t)blockIdx.x * a.run, tile1 = std::min<int64_t>(tile0 + a.run, tiles);
    const int d0 = (int)threadIdx.x * 4;
    int n_at = ragged_signal(a.sample_off, a.N, tile0 * kComposeTile), j_rec = -1, j_at = 0;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t t0 = tile * kComposeTile;
        const int span = (int)std::min<int64_t>(kComposeTile, a.total - t0);
        float v[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        while (n_at + 1 < a.N && a.sample_off[n_at + 1] <= t0) ++n_at;      // the last recording that starts at or before t0
        for (int n = n_at; n < a.N; ++n) {
            const int64_t r0 = a.sample_off[n];
            if (r0 - t0 >= span) break;
            // the recording's part of the tile [ra, rb); its sample i sits at tile position i - i0
            const int64_t i0 = t0 - r0;
            const int ra = r0 > t0 ? (int)(r0 - t0) : 0;
            const int rb = (int)std::min<int64_t>(a.sample_off[n + 1] - t0, span);
            if (rb <= ra) continue;
            float fg[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            const int pb = a.place_off[n + 1];
            const int pa = a.place_off[n];
            int j = pa, hi = pb;
            const int64_t i_lo = i0 + ra;
            if (n == j_rec) {                                // the first placement that ends behind the tile's first sample: a step or two on
                j = j_at;
                while (j < pb && a.place_first[j] + a.place_len[j] <= i_lo) ++j;
            } else {
                while (j < hi) {
                    const int mid = (j + hi) >> 1;
                    if (a.place_first[mid] + a.place_len[mid] > i_lo) hi = mid;
                    else j = mid + 1;
                }
            }
            for (; j < pb; ++j) {
                const int64_t st = a.place_first[j] - i0;   // the clip's first sample as a tile position
                if (st >= rb) break;
                const int ca = (int)std::max<int64_t>(st, ra), cb = (int)std::min<int64_t>(st + a.place_len[j], rb);
                if (cb <= ca) continue;
                const int64_t sb = a.place_clip_off[j] - st;
                const float gain = a.place_gain[j];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int d = d0 + h * 1024;
                    if (d + 3 < ca || d >= cb) continue;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (d + k >= ca && d + k < cb) fg[h][k] = (float)a.pcm[sb + d + k] * (1.0f / 32768.0f) * gain;
                }
            }
            j_rec = n;
            j_at = j > pa ? j - 1 : pa;
            const float vol = a.bg_vol ? a.bg_vol[n] : 0.f;
            const int64_t L = vol != 0.f ? a.bg_len[n] : 0;
            if (L >= 1) {
                int64_t base = (a.bg_phase[n] + i_lo) % L;  // the background position of tile position ra
                if (base < 0) base += L;
                const int64_t s1 = a.bg_off[n] + base - ra, s2 = s1 - L;
                const int wrap = ra + (int)std::min<int64_t>(L - base, kComposeTile);      // the first tile position past the loop's end
                const bool shorter = L < kComposeTile;
                const unsigned len32 = (unsigned)L, base32 = (unsigned)base;
                const int64_t s0 = a.bg_off[n];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int d = d0 + h * 1024;
                    if (d + 3 < ra || d >= rb) continue;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int e = d + k;
                        if (e < ra || e >= rb) continue;
                        const int64_t at = shorter ? s0 + (int64_t)((base32 + (unsigned)(e - ra)) % len32) : (e < wrap ? s1 : s2) + e;
                        v[h][k] = compose_mix((float)a.bg[at] * (1.0f / 32768.0f), vol, fg[h][k]);
                    }
                }
            } else {
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int e = d0 + h * 1024 + k;
                        if (e >= ra && e < rb) v[h][k] = fminf(fmaxf(fg[h][k], -1.0f), 1.0f);
                    }
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int d = d0 + h * 1024;
            if (d >= span) continue;
            const int64_t p = t0 + d;
            if (d + 4 <= span) {
                if (a.out) mine_store4(a.out + p, v[h][0], v[h][1], v[h][2], v[h][3]);
                if (a.out_pcm) mine_store4(a.out_pcm + p, v[h][0], v[h][1], v[h][2], v[h][3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (d + k >= span) break;
                    if (a.out) a.out[p + k] = v[h][k];
                    if (a.out_pcm) a.out_pcm[p + k] = mine_pcm(v[h][k]);
                }
            }
        }
    }
}

struct EnergyArgs {
    const int16_t* pcm;
    const int64_t* clip_off;    // [n]
    const int64_t* clip_len;
    int64_t* sumsq;             // [n], zeroed
    int64_t n;
};

struct alignas(16) EnergyPcm8 { int16_t v[8]; };

// x^2 + y^2 <= 2^31: the sum in unsigned arithmetic (it does not fit an int)
__device__ __forceinline__ uint64_t energy_sq2(int x, int y) { return (uint64_t)((unsigned)(x * x) + (unsigned)(y * y)); }

// The workgroup's total in thread 0.
__device__ __forceinline__ uint64_t energy_block_sum(uint64_t mine) {
    __shared__ uint64_t s_sum[256];
    const int tid = threadIdx.x;
    __syncthreads();                                    // (the previous group's total has been read)
    s_sum[tid] = mine;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
    }
    return s_sum[0];
}

// Clip j: `head` samples in front of its first 16-byte-aligned element, `chunks` aligned runs of eight, the rest behind them.
struct EnergyClip {
    const int16_t* src;
    int64_t len, chunks;
    int head;
};

__device__ __forceinline__ EnergyClip energy_clip(const EnergyArgs& a, int64_t j) {
    EnergyClip c;
    c.src = a.pcm + a.clip_off[j];
    c.len = std::max<int64_t>(a.clip_len[j], 0);
    c.head = (int)std::min<int64_t>((16 - (int)(reinterpret_cast<uintptr_t>(c.src) & 15)) & 15, 2 * c.len) / 2;
    c.chunks = (c.len - c.head) / 8;
    return c;
}

// Group g of clip c (its aligned runs g kEnergyGroup .. + kEnergyGroup - 1; group 0 also the unaligned ends), added to sumsq[j].
__device__ __forceinline__ void energy_group(const EnergyArgs& a, const EnergyClip& c, int64_t j, int64_t g) {
    const int tid = threadIdx.x;
    const int64_t c0 = g * kEnergyGroup;
    const int cn = (int)std::min<int64_t>(c.chunks - c0, kEnergyGroup);
    const int16_t* at = c.src + c.head + 8 * c0;
    uint64_t sum = 0;
    for (int q = tid; q < cn; q += 256) {
        const EnergyPcm8 u = *reinterpret_cast<const EnergyPcm8*>(at + 8 * q);
        sum += energy_sq2(u.v[0], u.v[1]) + energy_sq2(u.v[2], u.v[3]) + energy_sq2(u.v[4], u.v[5]) + energy_sq2(u.v[6], u.v[7]);
    }
    if (g == 0) {
        const int64_t tail = c.head + 8 * c.chunks;
        const int rest = c.head + (int)(c.len - tail);  // at most 7 + 7
        if (tid < rest) {
            const int x = c.src[tid < c.head ? tid : tail + tid - c.head];
            sum += (uint64_t)(unsigned)(x * x);
        }
    }
    const uint64_t all = energy_block_sum(sum);
    if (tid == 0 && all) __atomic_fetch_add(reinterpret_cast<uint64_t*>(a.sumsq + j), all, __ATOMIC_RELAXED);
}

// Workgroups 0 .. n - 1: clip j's group 0.  Behind them kEnergyParts workgroups per 64 clips: part r takes the groups
// 1 + r, 1 + r + kEnergyParts, .. of those of the 64 that have more than one.
__global__ __launch_bounds__(256) void pcm_energy_kernel(const EnergyArgs a) {
    const int64_t b = blockIdx.x;
    if (b < a.n) {
        energy_group(a, energy_clip(a, b), b, 0);
        return;
    }
    const int64_t set = (b - a.n) / kEnergyParts;
    const int part = (int)((b - a.n) - set * kEnergyParts);
    for (int64_t j = set * 64; j < std::min<int64_t>(set * 64 + 64, a.n); ++j) {
        if (a.clip_len[j] <= 8 * kEnergyGroup) continue;        // (one group at most)
        const EnergyClip c = energy_clip(a, j);
        const int64_t groups = (c.chunks + kEnergyGroup - 1) / kEnergyGroup;
        for (int64_t g = 1 + part; g < groups; g += kEnergyParts) energy_group(a, c, j, g);
    }
}

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_pcm_energy(const int16_t* pcm, const int64_t* clip_off, const int64_t* clip_len, int64_t n_clips, int64_t* sumsq,
                              void* stream) {
    const char* what = "tcr_pcm_energy";
    TCR_REQUIRE(n_clips >= 0, "%s: n_clips must be >= 0 (got %lld)", what, (long long)n_clips);
    if (n_clips == 0) return TCR_OK;
    TCR_REQUIRE(pcm && clip_off && clip_len && sumsq, "%s: null argument", what);
    const int64_t blocks = n_clips + ceil_div64(n_clips, 64) * kEnergyParts;
    TCR_REQUIRE(blocks < ((int64_t)1 << 31), "%s: %lld clips are too many for one launch", what, (long long)n_clips);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(sumsq, 0, (size_t)n_clips * sizeof(int64_t), s) != hipSuccess) {
        set_error("%s: hipMemsetAsync of sumsq failed", what);
        return TCR_ERR_HIP;
    }
    EnergyArgs a{};
    a.pcm = pcm; a.clip_off = clip_off; a.clip_len = clip_len; a.sumsq = sumsq; a.n = n_clips;
    hipLaunchKernelGGL(pcm_energy_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return check_launch("pcm_energy_kernel");
}

extern "C" int tcr_compose(int n_signals, const int64_t* sample_offsets, int64_t total_samples, const int16_t* pcm,
                           const int32_t* place_offsets, const int64_t* place_clip_off, const int32_t* place_len, const int64_t* place_first,
                           const float* place_gain, const int16_t* bg, const int64_t* bg_off, const int64_t* bg_len, const int64_t* bg_phase,
                           const float* bg_vol, float* out, int16_t* out_pcm, void* stream) {
    const char* what = "tcr_compose";
    TCR_REQUIRE(out || out_pcm, "%s: out and out_pcm are both null", what);
    TCR_REQUIRE(n_signals > 0, "%s: the number of signals must be positive (got %d)", what, n_signals);
    TCR_REQUIRE(total_samples >= 0, "%s: total_samples must be >= 0 (got %lld)", what, (long long)total_samples);
    TCR_REQUIRE(sample_offsets && pcm && place_offsets && place_clip_off && place_len && place_first && place_gain, "%s: null argument", what);
    TCR_REQUIRE(!bg_vol || (bg && bg_off && bg_len && bg_phase), "%s: bg_vol given without bg / bg_off / bg_len / bg_phase", what);
    TCR_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "%s: out must be 16-byte aligned", what);
    TCR_REQUIRE((reinterpret_cast<uintptr_t>(out_pcm) & 7) == 0, "%s: out_pcm must be 8-byte aligned", what);
    if (total_samples == 0) return TCR_OK;
    const int64_t tiles = ceil_div64(total_samples, kComposeTile);
    TCR_REQUIRE(tiles < ((int64_t)1 << 31), "%s: %lld samples are too many for one launch", what, (long long)total_samples);
    ComposeArgs a{};
    a.sample_off = sample_offsets; a.pcm = pcm; a.place_off = place_offsets; a.place_clip_off = place_clip_off; a.place_len = place_len;
    a.place_first = place_first; a.place_gain = place_gain; a.bg = bg; a.bg_off = bg_off; a.bg_len = bg_len; a.bg_phase = bg_phase;
    a.bg_vol = bg_vol; a.out = out; a.out_pcm = out_pcm; a.total = total_samples; a.N = n_signals;
    const int knob = tune_get(TCR_TUNE_COMPOSE_RUN);
    a.run = knob > 0 ? knob : kComposeRun;
    hipLaunchKernelGGL(compose_kernel, dim3((unsigned)ceil_div64(tiles, a.run)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("compose_kernel");
}
