// Hard-example mining over a scan (tcr_mine_detections, tcr_mine_peaks, tcr_mine_select, tcr_mine_gather): which windows fired outside
// any event, which events were never hit, which windows came close, the K best of them, and their audio.
//
// Every in-order compaction is scan_select.hip's three-phase prefix sum over tiles of kSelTile items (select_count_kernel,
// select_scan_kernel, select_prefix_kernel, select_compact_kernel and their helpers select_tile_bits / select_block_prefix): a byte per
// item in the workspace, the tiles' sums, one workgroup scanning the sums.  No workgroup waits for another (every dependence between
// workgroups is a kernel boundary) and no output position comes from an atomic: the results are deterministic, in item order.
//
// tcr_mine_detections: the hit / duplicate / false-accept rule of sweep.hip without its sequential walk.  Events are sorted and
// disjoint and an event has one label, so "no earlier detection hit event e" means: this is the first is_new step in e's range whose
// top is e's label.
//   mine_det_flag_kernel      a byte per step: is_new != 0 and 0 <= top < C;
//   select_count_kernel, select_scan_kernel (n_cand), select_compact_kernel: cand_step;
//   mine_event_kernel         a wave per event: the first flagged step of its range with its label, 64 steps a probe (event_hit);
//   mine_classify_kernel      a thread per candidate: its signal and the event that covers it by two binary searches, its kind by
//                             comparing its step with event_hit.
// tcr_mine_peaks: local maxima of values[.][c] within R steps of their own signal.
//   mine_peak_kernel          a workgroup per tile of TCR_MINE_TILE steps stages the tile and R steps on both sides in LDS, a chunk of
//                             classes at a time, cuts the staged steps into blocks of R and walks every (block, class) once up and once
//                             down: the running maximum since the block's (or the signal's) first step and until its last.  A window
//                             of at most R steps lies in one block or two adjacent ones, so its maximum is one or two of those values
//                             whatever R.  NaN is the empty maximum (fmaxf ignores it), so NaN neighbours and empty windows need no case;
//   select_count_kernel, select_scan_kernel (n_cand: the true count), mine_peak_emit_kernel (select_compact_kernel's positions, up to
//                             `capacity`): the tables in (step, class) order.
// tcr_mine_select: radix select.  key = the order-preserving unsigned image of the float (-0 as +0).  Four passes over the keys' bytes
// from the top: mine_hist_kernel counts, per value of the byte, the eligible candidates whose higher bytes equal the prefix found so
// far (LDS counters, then one integer add per workgroup and value: sums, so their order does not matter), mine_digit_kernel walks the
// 256 counts from the top and fixes the byte that holds the K-th largest.  Then the ties at the K-th key are ranked by
// select_prefix_kernel, mine_pick_kernel flags everything above the key and the first ties, and one compaction writes `picked`.
// tcr_mine_gather: a row per clip, 16-byte stores at the row's aligned elements; their four source floats come from one or two aligned
// 16-byte loads (the shift between source and destination is one number per clip), elements next to the signal's ends and the row's
// unaligned head and tail go one by one with a bounds check.  int16 rows: the same loads, 8-byte stores.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after scan_select.hip).
#pragma once
#include <algorithm>
#include <cmath>

namespace tcr {

namespace {

constexpr int kMineTile = TCR_MINE_TILE;
constexpr int kMineLdsBytes = 63 * 1024;                // dynamic LDS of mine_peak_kernel
constexpr int kMineRadiusMax = (kMineLdsBytes / 12 - kMineTile) / 2;       // one class a chunk: 12 bytes per staged step
static_assert(kMineRadiusMax == TCR_MINE_RADIUS_MAX, "include/tcresnet_hip.h states the bound");
constexpr int kMineItems = 16;                          // candidates per thread of mine_hist_kernel

}  // namespace

struct MineDetArgs {
    const int32_t* top;         // [total]
    const float* score;
    const int32_t* is_new;
    const int64_t* step_off;    // [N + 1]
    const int32_t* ev_off;      // [N + 1] or null
    const int64_t* ev_first;
    const int64_t* ev_last;
    const int32_t* ev_label;
    uint8_t* bits;              // [total]
    const int64_t* cand_step;   // (select_compact_kernel wrote it)
    const int64_t* n_cand;
    int32_t* cand_label;
    float* cand_value;
    uint8_t* cand_kind;
    int32_t* cand_event;
    int64_t* event_hit;         // [E]
    int64_t total;
    int N, C, E;
};

__global__ __launch_bounds__(256) void mine_det_flag_kernel(const MineDetArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.total) return;
    const int c = a.top[p];
    a.bits[p] = a.is_new[p] != 0 && c >= 0 && c < a.C ? 1 : 0;
}

// the last n in 0 .. n_sig - 1 with off[n] <= v (int32 offsets: the events' CSR)
__device__ __forceinline__ int mine_csr_row(const int32_t* off, int n_sig, int v) {
    int lo = 0, hi = n_sig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A wave per event: the first flagged step of the event's range (clamped to its signal's steps) whose top is the event's label.
__global__ __launch_bounds__(256) void mine_event_kernel(const MineDetArgs a) {
    const int lane = threadIdx.x & 63;
    const int e = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= a.E) return;
    const int n = mine_csr_row(a.ev_off, a.N, e);
    const int64_t row0 = a.step_off[n], steps = a.step_off[n + 1] - row0;
    const int lab = a.ev_label[e];
    int64_t f = a.ev_first[e], l = a.ev_last[e];
    if (f < 0) f = 0;
    if (l > steps - 1) l = steps - 1;
    int64_t hit = -1;
    if (e < a.ev_off[n + 1] && lab >= 0 && lab < a.C) {
        for (int64_t s = f; s <= l; s += 64) {
            const int64_t p = row0 + s + lane;
            int m = 64;
            if (s + lane <= l && a.bits[p] && a.top[p] == lab) m = lane;
#pragma unroll
            for (int k = 1; k < 64; k <<= 1) m = min(m, __shfl_xor(m, k));
            if (m < 64) {
                hit = row0 + s + m;
                break;
            }
        }
    }
    if (lane == 0) a.event_hit[e] = hit;
}

// A thread per candidate (a grid-stride loop up to the count the scan wrote).
__global__ __launch_bounds__(256) void mine_classify_kernel(const MineDetArgs a) {
    const int64_t n_cand = *a.n_cand;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n_cand; j += (int64_t)gridDim.x * 256) {
        const int64_t p = a.cand_step[j];
        const int lab = a.top[p];
        a.cand_label[j] = lab;
        a.cand_value[j] = a.score[p];
        int ev = -1, kind = 0;
        if (a.ev_off) {
            const int n = ragged_signal(a.step_off, a.N, p);
            const int64_t i = p - a.step_off[n];
            int lo = a.ev_off[n], hi = a.ev_off[n + 1];         // the last event of the signal that starts at or before i
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (a.ev_first[mid] <= i) lo = mid + 1;
                else hi = mid;
            }
            if (lo > a.ev_off[n] && a.ev_last[lo - 1] >= i) {
                ev = lo - 1;
                if (a.ev_label[ev] == lab) kind = a.event_hit[ev] == p ? 1 : 2;
            }
        }
        a.cand_kind[j] = (uint8_t)kind;
        a.cand_event[j] = ev;
    }
}

struct MinePeakArgs {
    const float* values;        // [total][C]
    const uint8_t* class_mask;  // [C]
    const int64_t* step_off;    // [N + 1]
    const int32_t* ex_off;      // [N + 1] or null
    const int64_t* ex_first;
    const int64_t* ex_last;
    uint8_t* bits;              // [total][C]
    int64_t* cand_step;
    int32_t* cand_label;
    float* cand_value;
    int64_t total, capacity;
    int N, C, R, CC;            // CC: classes per staged chunk
    float floor;
};

// Dynamic LDS: g [S][CC] floats (the staged values, then the running maxima upwards), h [S][CC] (downwards), sig [S] ints, S = tile + 2 R.
__global__ __launch_bounds__(256) void mine_peak_kernel(const MinePeakArgs a) {
    const int R = a.R, C = a.C, CC = a.CC, S = kMineTile + 2 * R, tid = threadIdx.x;
    float* s_g = reinterpret_cast<float*>(dyn_lds());
    float* s_h = s_g + (size_t)S * CC;
    int* s_sig = reinterpret_cast<int*>(s_h + (size_t)S * CC);
    const int64_t t0 = (int64_t)blockIdx.x * kMineTile, base = t0 - R;
    for (int s = tid; s < S; s += 256) {
        const int64_t q = base + s;
        s_sig[s] = q >= 0 && q < a.total ? ragged_signal(a.step_off, a.N, q) : -1;
    }
    const int nb = (S + R - 1) / R;
    for (int c0 = 0; c0 < C; c0 += CC) {
        const int cn = C - c0 < CC ? C - c0 : CC;
        __syncthreads();
        for (int e = tid; e < S * cn; e += 256) {
            const int s = e / cn, cc = e - s * cn;
            float v = __builtin_nanf("");
            if (s_sig[s] >= 0) v = a.values[(base + s) * C + c0 + cc];
            s_g[s * CC + cc] = v;
        }
        __syncthreads();
        for (int w = tid; w < nb * cn; w += 256) {
            const int b = w / cn, cc = w - b * cn;
            const int lo = b * R, hi = (lo + R < S ? lo + R : S) - 1;
            float m = __builtin_nanf("");
            int sg = -2;
            for (int s = hi; s >= lo; --s) {
                if (s_sig[s] != sg) { m = __builtin_nanf(""); sg = s_sig[s]; }
                m = fmaxf(m, s_g[s * CC + cc]);
                s_h[s * CC + cc] = m;
            }
            m = __builtin_nanf("");
            sg = -2;
            for (int s = lo; s <= hi; ++s) {
                if (s_sig[s] != sg) { m = __builtin_nanf(""); sg = s_sig[s]; }
                m = fmaxf(m, s_g[s * CC + cc]);
                s_g[s * CC + cc] = m;
            }
        }
        __syncthreads();
        for (int e = tid; e < kMineTile * cn; e += 256) {
            const int ls = e / cn, cc = e - ls * cn, c = c0 + cc;
            const int64_t p = t0 + ls;
            if (p >= a.total) break;
            bool ok = false;
            if (a.class_mask[c] != 0) {
                const float v = a.values[p * C + c];
                if (v >= a.floor) {
                    const int s = ls + R, n = s_sig[s];
                    const int64_t row0 = a.step_off[n], end = a.step_off[n + 1];
                    const int64_t lo = p - R > row0 ? p - R : row0, hi = p + R < end - 1 ? p + R : end - 1;
                    ok = true;
                    if (lo < p) {                               // the maximum over lo .. p - 1
                        const int sl = (int)(lo - base), sr = s - 1;
                        const float g = s_g[sr * CC + cc];
                        const float m = sl / R == sr / R ? g : fmaxf(s_h[sl * CC + cc], g);
                        ok = !(m >= v);
                    }
                    if (ok && hi > p) {                         // over p + 1 .. hi
                        const int sl = s + 1, sr = (int)(hi - base);
                        const float h = s_h[sl * CC + cc];
                        const float m = sl / R == sr / R ? h : fmaxf(h, s_g[sr * CC + cc]);
                        ok = !(m > v);
                    }
                    if (ok && a.ex_off) {
                        const int64_t i = p - row0;
                        int xl = a.ex_off[n], xh = a.ex_off[n + 1];
                        while (xl < xh) {
                            const int mid = (xl + xh) >> 1;
                            if (a.ex_first[mid] <= i) xl = mid + 1;
                            else xh = mid;
                        }
                        if (xl > a.ex_off[n] && a.ex_last[xl - 1] >= i) ok = false;
                    }
                }
            }
            a.bits[p * C + c] = ok ? 1 : 0;
        }
    }
}

// select_compact_kernel's positions over the (step, class) flags; the first `capacity` candidates are stored.
__global__ __launch_bounds__(256) void mine_peak_emit_kernel(const SelectArgs a, const MinePeakArgs m) {
    int v[4], total;
    const int64_t at = select_tile_bits(a, v);
    int64_t out = a.sums[blockIdx.x] + select_block_prefix(v[0] + v[1] + v[2] + v[3], total);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!v[e]) continue;
        if (out < m.capacity) {
            const int64_t x = at + e, p = x / m.C;
            m.cand_step[out] = p;
            m.cand_label[out] = (int32_t)(x - p * m.C);
            m.cand_value[out] = m.values[x];
        }
        ++out;
    }
}

struct MinePickArgs {
    const float* value;         // [n]
    const uint8_t* kind;        // [n] or null
    uint8_t* bits;              // [n]
    const int32_t* prefix;      // [n]: the ties in 0 .. j
    unsigned* hist;             // [4][256]
    unsigned* state;            // [0] the key's bytes found so far, [1] the candidates still wanted among those that share them
    int64_t n;
    unsigned kind_mask, k;
    int pass;
};

// larger float <=> larger key; -0 and +0 share one
__device__ __forceinline__ unsigned mine_key(float v) {
    unsigned u = __builtin_bit_cast(unsigned, v);
    if (u == 0x80000000u) u = 0;
    return u & 0x80000000u ? ~u : u | 0x80000000u;
}

__device__ __forceinline__ bool mine_eligible(const MinePickArgs& a, int64_t j) {
    return !a.kind || ((a.kind_mask >> (a.kind[j] & 31)) & 1u) != 0;
}

__global__ __launch_bounds__(256) void mine_hist_kernel(const MinePickArgs a) {
    __shared__ int s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int shift = 24 - 8 * a.pass;
    const unsigned want = a.pass ? a.state[0] >> (shift + 8) : 0;
    const int64_t first = (int64_t)blockIdx.x * 256 * kMineItems + threadIdx.x;
#pragma unroll 4
    for (int e = 0; e < kMineItems; ++e) {
        const int64_t j = first + e * 256;
        if (j >= a.n || !mine_eligible(a, j)) continue;
        const unsigned key = mine_key(a.value[j]);
        if (a.pass && key >> (shift + 8) != want) continue;
        atomicAdd(&s_hist[(key >> shift) & 255], 1);
    }
    __syncthreads();
    const int mine = s_hist[threadIdx.x];
    if (mine) atomicAdd(&a.hist[a.pass * 256 + threadIdx.x], (unsigned)mine);
}

// One workgroup.  Thread t looks at byte value 255 - t: the byte whose count reaches the candidates still wanted is the key's.
// Pass 0 with fewer eligible candidates than k: everything is taken (state[1] = 0xffffffff, the key 0).
__global__ __launch_bounds__(256) void mine_digit_kernel(const MinePickArgs a) {
    const int shift = 24 - 8 * a.pass;
    const int mine = (int)a.hist[a.pass * 256 + 255 - threadIdx.x];
    int all;
    const int above = select_block_prefix(mine, all);
    const unsigned want = a.pass ? a.state[1] : a.k;
    __syncthreads();                                    // (every thread has read the state)
    if (a.pass == 0 && (unsigned)all < want) {
        if (threadIdx.x == 0) { a.state[0] = 0; a.state[1] = 0xffffffffu; }
        return;
    }
    if (want == 0xffffffffu) return;
    if ((unsigned)above < want && want <= (unsigned)(above + mine)) {
        a.state[0] = (a.pass ? a.state[0] : 0) | (unsigned)(255 - threadIdx.x) << shift;
        a.state[1] = want - (unsigned)above;
    }
}

// TIES: a byte per candidate, 1 where it is eligible and its key is the K-th; else the picks: above the key, or a tie among the first.
template <bool TIES>
__global__ __launch_bounds__(256) void mine_pick_kernel(const MinePickArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const unsigned kth = a.state[0], ties = a.state[1];
    int f = 0;
    if (mine_eligible(a, j)) {
        const unsigned key = mine_key(a.value[j]);
        if (TIES) f = key == kth;
        else f = key > kth || (key == kth && (unsigned)a.prefix[j] <= ties);
    }
    a.bits[j] = (uint8_t)f;
}

struct MineGatherArgs {
    const float* samples;       // packed
    const int64_t* sample_off;  // [N + 1]
    const int32_t* clip_signal; // [n]
    const int64_t* clip_first;
    float* out;                 // [n][n_samples] or null
    int16_t* out_pcm;
    int n_samples, N, parts;
};

struct alignas(8) MinePcm4 { int16_t x, y, z, w; };

// clamp(rint(32768 x), -32768, 32767), ties to even, NaN -> 0: the inverse of the int16 decode v / 32768
__device__ __forceinline__ int16_t mine_pcm(float x) {
    float y = rintf(x * 32768.f);
    y = y > 32767.f ? 32767.f : y;
    y = y < -32768.f ? -32768.f : y;
    return (int16_t)(int)(x != x ? 0.f : y);
}

__device__ __forceinline__ void mine_store4(float* d, float x0, float x1, float x2, float x3) {
    *reinterpret_cast<float4*>(d) = make_float4(x0, x1, x2, x3);
}
__device__ __forceinline__ void mine_store4(int16_t* d, float x0, float x1, float x2, float x3) {
    *reinterpret_cast<MinePcm4*>(d) = MinePcm4{mine_pcm(x0), mine_pcm(x1), mine_pcm(x2), mine_pcm(x3)};
}
__device__ __forceinline__ void mine_store1(float* d, float x) { *d = x; }
__device__ __forceinline__ void mine_store1(int16_t* d, float x) { *d = mine_pcm(x); }

// The aligned chunks of a row (see mine_gather_row): chunk c is d[head + 4 c .. + 3].  SHIFTED: the source is `shift` = 1 .. 3 floats past
// a 16-byte boundary there, so the four floats straddle two aligned source chunks; else they are one.
template <class OutT, bool SHIFTED>
__device__ __forceinline__ void mine_gather_chunks(const float* src, int64_t len, int64_t first, OutT* d, int head, int chunks, int shift,
                                                   int part, int parts) {
    for (int c = part * 256 + (int)threadIdx.x; c < chunks; c += parts * 256) {
        const int e = head + 4 * c;
        const int64_t pos = first + e, pa = pos - shift;           // src + pa is 16-byte aligned
        float x0, x1, x2, x3;
        if (pa >= 0 && pa + (SHIFTED ? 8 : 4) <= len) {
            const float4 u = *reinterpret_cast<const float4*>(src + pa);
            if constexpr (SHIFTED) {
                // (selects, not branches: a branch per shift lets the compiler cut the two loads into the dwords that branch uses)
                const float4 w = *reinterpret_cast<const float4*>(src + pa + 4);
                const bool s1 = shift == 1, s2 = shift == 2;
                x0 = s1 ? u.y : s2 ? u.z : u.w;
                x1 = s1 ? u.z : s2 ? u.w : w.x;
                x2 = s1 ? u.w : s2 ? w.x : w.y;
                x3 = s1 ? w.x : s2 ? w.y : w.z;
            } else {
                x0 = u.x; x1 = u.y; x2 = u.z; x3 = u.w;
            }
        } else {
            x0 = pos >= 0 && pos < len ? src[pos] : 0.f;
            x1 = pos + 1 >= 0 && pos + 1 < len ? src[pos + 1] : 0.f;
            x2 = pos + 2 >= 0 && pos + 2 < len ? src[pos + 2] : 0.f;
            x3 = pos + 3 >= 0 && pos + 3 < len ? src[pos + 3] : 0.f;
        }
        mine_store4(d + e, x0, x1, x2, x3);
    }
}

// Row d[0 .. n) <- src[first .. first + n) of a signal of len samples, zeros outside it; this workgroup is part `part` of `parts`.
template <class OutT>
__device__ __forceinline__ void mine_gather_row(const float* src, int64_t len, int64_t first, OutT* d, int n, int part, int parts) {
    constexpr int kAlign = 4 * (int)sizeof(OutT);
    const int tid = threadIdx.x;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(d) & (kAlign - 1));
    int head = (int)(((kAlign - mis) & (kAlign - 1)) / sizeof(OutT));
    if (head > n) head = n;
    const int chunks = (n - head) / 4, tail = head + 4 * chunks;
    const int shift = (int)((((int64_t)(reinterpret_cast<uintptr_t>(src) >> 2)) + first + head) & 3);
    if (shift == 0) mine_gather_chunks<OutT, false>(src, len, first, d, head, chunks, 0, part, parts);
    else mine_gather_chunks<OutT, true>(src, len, first, d, head, chunks, shift, part, parts);
    if (part == 0) {                                            // the unaligned head and tail: at most 3 + 3 elements
        const int rest = head + (n - tail);
        if (tid < rest) {
            const int e = tid < head ? tid : tail + tid - head;
            const int64_t pos = first + e;
            mine_store1(d + e, pos >= 0 && pos < len ? src[pos] : 0.f);
        }
    }
}

// `parts` workgroups per clip.  A clip whose signal index is outside 0 .. N - 1 reads nothing and is all zeros.
__global__ __launch_bounds__(256) void mine_gather_kernel(const MineGatherArgs a) {
    const int64_t i = blockIdx.x / (unsigned)a.parts;
    const int part = (int)(blockIdx.x - (unsigned)i * a.parts);
    const int sig = a.clip_signal[i];
    const float* src = a.samples;
    int64_t len = 0;
    if (sig >= 0 && sig < a.N) {
        const int64_t o = a.sample_off[sig];
        src = a.samples + o;
        len = a.sample_off[sig + 1] - o;
        if (len < 0) len = 0;
    }
    const int64_t first = a.clip_first[i];
    if (a.out) mine_gather_row(src, len, first, a.out + i * a.n_samples, a.n_samples, part, a.parts);
    if (a.out_pcm) mine_gather_row(src, len, first, a.out_pcm + i * a.n_samples, a.n_samples, part, a.parts);
}

namespace {

struct MineWs {
    uint8_t* bits;
    int32_t* prefix;
    int32_t* sums;
    unsigned* hist;             // [4][256], then the two state words
    size_t bytes;
};

// the workspace of n items: bits | sums | hist + state | prefix (RANKED only: tcr_mine_select's tie ranks)
MineWs mine_ws(void* base, int64_t n, bool ranked) {
    MineWs w;
    const int64_t tiles = ceil_div64(n, kSelTile);
    char* p = static_cast<char*>(base);
    w.bits = reinterpret_cast<uint8_t*>(p);
    p += round_up64(n, 256);
    w.sums = reinterpret_cast<int32_t*>(p);
    p += round_up64((tiles + 1) * 4, 256);
    w.hist = reinterpret_cast<unsigned*>(p);
    p += (4 * 256 + 64) * sizeof(unsigned);
    w.prefix = reinterpret_cast<int32_t*>(p);
    if (ranked) p += round_up64(n * 4, 256);
    w.bytes = (size_t)(p - static_cast<char*>(base));
    return w;
}

int mine_ws_check(const char* what, int64_t n, bool ranked, size_t ws_bytes) {
    const size_t need = mine_ws(nullptr, n, ranked).bytes;
    if (ws_bytes < need) {
        set_error("%s: workspace %zu bytes < %zu for %lld items", what, ws_bytes, need, (long long)n);
        return TCR_ERR_WORKSPACE;
    }
    return TCR_OK;
}

// the flags in w.bits -> their number in *count; COMPACT: and their indices, increasing, in `selected`
SelectArgs mine_select_args(const MineWs& w, int64_t n, int64_t* selected, int64_t* count) {
    SelectArgs a{};
    a.bits = w.bits; a.prefix = w.prefix; a.sums = w.sums; a.selected = selected; a.n_selected = count; a.total = n;
    a.tiles = (int)ceil_div64(n, kSelTile);
    return a;
}

int mine_count_scan(const SelectArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(select_count_kernel, dim3(a.tiles), dim3(256), 0, s, a);
    TCR_TRY(check_launch("select_count_kernel"));
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, s, a);
    return check_launch("select_scan_kernel");
}

unsigned mine_stride_blocks(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(n, 256), 16 * (int64_t)device_cus()));
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" size_t tcr_mine_workspace_bytes(int64_t n_items, int ranked) {
    if (n_items <= 0 || n_items >= ((int64_t)1 << 31)) {
        set_error("tcr_mine_workspace_bytes: n_items %lld outside 1..2^31 - 1", (long long)n_items);
        return 0;
    }
    return mine_ws(nullptr, n_items, ranked != 0).bytes;
}

extern "C" int tcr_mine_detections(int n_signals, const int64_t* step_offsets, int64_t total_steps, int num_classes, const int32_t* top,
                                   const float* score, const int32_t* is_new, const int32_t* event_offsets, const int64_t* event_first,
                                   const int64_t* event_last, const int32_t* event_label, int n_events, void* workspace, size_t ws_bytes,
                                   int64_t* cand_step, int32_t* cand_label, float* cand_value, uint8_t* cand_kind, int32_t* cand_event,
                                   int64_t* n_cand, int64_t* event_hit, void* stream) {
    const char* what = "tcr_mine_detections";
    TCR_REQUIRE(step_offsets && top && score && is_new && workspace && cand_step && cand_label && cand_value && cand_kind && cand_event &&
                n_cand, "%s: null argument", what);
    TCR_TRY(detect_shape_check(what, true, n_signals, 0, total_steps, num_classes));
    TCR_REQUIRE(!event_offsets || (event_first && event_last && event_label && n_events >= 0 && (n_events == 0 || event_hit)),
                "%s: events need event_first, event_last, event_label, n_events >= 0 and event_hit", what);
    TCR_TRY(mine_ws_check(what, total_steps, false, ws_bytes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MineWs w = mine_ws(workspace, total_steps, false);
    MineDetArgs a{};
    a.top = top; a.score = score; a.is_new = is_new; a.step_off = step_offsets;
    a.ev_off = event_offsets; a.ev_first = event_first; a.ev_last = event_last; a.ev_label = event_label;
    a.bits = w.bits; a.cand_step = cand_step; a.n_cand = n_cand; a.cand_label = cand_label; a.cand_value = cand_value;
    a.cand_kind = cand_kind; a.cand_event = cand_event; a.event_hit = event_hit;
    a.total = total_steps; a.N = n_signals; a.C = num_classes; a.E = event_offsets ? n_events : 0;
    hipLaunchKernelGGL(mine_det_flag_kernel, dim3((unsigned)ceil_div64(total_steps, 256)), dim3(256), 0, s, a);
    TCR_TRY(check_launch("mine_det_flag_kernel"));
    const SelectArgs sa = mine_select_args(w, total_steps, cand_step, n_cand);
    TCR_TRY(mine_count_scan(sa, s));
    hipLaunchKernelGGL(select_compact_kernel, dim3(sa.tiles), dim3(256), 0, s, sa);
    TCR_TRY(check_launch("select_compact_kernel"));
    if (a.E > 0) {
        hipLaunchKernelGGL(mine_event_kernel, dim3((unsigned)ceil_div64(a.E, 4)), dim3(256), 0, s, a);
        TCR_TRY(check_launch("mine_event_kernel"));
    }
    hipLaunchKernelGGL(mine_classify_kernel, dim3(mine_stride_blocks(total_steps)), dim3(256), 0, s, a);
    return check_launch("mine_classify_kernel");
}

extern "C" int tcr_mine_peaks(int n_signals, const int64_t* step_offsets, int64_t total_steps, int num_classes, const float* values,
                              const uint8_t* class_mask, float floor, int radius, const int32_t* exclude_offsets,
                              const int64_t* exclude_first, const int64_t* exclude_last, void* workspace, size_t ws_bytes, int64_t capacity,
                              int64_t* cand_step, int32_t* cand_label, float* cand_value, int64_t* n_cand, void* stream) {
    const char* what = "tcr_mine_peaks";
    TCR_REQUIRE(step_offsets && values && class_mask && workspace && n_cand, "%s: null argument", what);
    TCR_TRY(detect_shape_check(what, true, n_signals, 0, total_steps, num_classes));
    TCR_REQUIRE(floor == floor, "%s: floor is NaN", what);
    TCR_REQUIRE(radius >= 1 && radius <= kMineRadiusMax, "%s: radius %d outside 1..%d", what, radius, kMineRadiusMax);
    TCR_REQUIRE(capacity >= 0, "%s: capacity must be >= 0 (got %lld)", what, (long long)capacity);
    TCR_REQUIRE(capacity == 0 || (cand_step && cand_label && cand_value), "%s: null candidate tables with capacity %lld", what,
                (long long)capacity);
    TCR_REQUIRE(!exclude_offsets || (exclude_first && exclude_last), "%s: exclusion ranges need exclude_first and exclude_last", what);
    const int64_t pairs = total_steps * num_classes;
    TCR_TRY(mine_ws_check(what, pairs, false, ws_bytes));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const MineWs w = mine_ws(workspace, pairs, false);
    MinePeakArgs a{};
    a.values = values; a.class_mask = class_mask; a.step_off = step_offsets;
    a.ex_off = exclude_offsets; a.ex_first = exclude_first; a.ex_last = exclude_last;
    a.bits = w.bits; a.cand_step = cand_step; a.cand_label = cand_label; a.cand_value = cand_value;
    a.total = total_steps; a.capacity = capacity; a.N = n_signals; a.C = num_classes; a.R = radius; a.floor = floor;
    const int staged = kMineTile + 2 * radius;
    a.CC = std::min(num_classes, (kMineLdsBytes / staged - 4) / 8);
    const size_t lds = (size_t)staged * (8 * a.CC + 4);
    if (lds > 32 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(mine_peak_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds) != hipSuccess) {
        set_error("%s: hipFuncSetAttribute failed", what);
        return TCR_ERR_HIP;
    }
    hipLaunchKernelGGL(mine_peak_kernel, dim3((unsigned)ceil_div64(total_steps, kMineTile)), dim3(256), lds, s, a);
    TCR_TRY(check_launch("mine_peak_kernel"));
    const SelectArgs sa = mine_select_args(w, pairs, nullptr, n_cand);
    TCR_TRY(mine_count_scan(sa, s));
    hipLaunchKernelGGL(mine_peak_emit_kernel, dim3(sa.tiles), dim3(256), 0, s, sa, a);
    return check_launch("mine_peak_emit_kernel");
}

extern "C" int tcr_mine_select(int64_t n_cand, const float* cand_value, const uint8_t* cand_kind, uint32_t kind_mask, int64_t k,
                               void* workspace, size_t ws_bytes, int64_t* picked, int64_t* n_picked, void* stream) {
    const char* what = "tcr_mine_select";
    TCR_REQUIRE(n_picked, "%s: null argument", what);
    TCR_REQUIRE(n_cand >= 0 && n_cand < ((int64_t)1 << 31), "%s: n_cand %lld outside 0..2^31 - 1", what, (long long)n_cand);
    TCR_REQUIRE(k >= 0, "%s: k must be >= 0 (got %lld)", what, (long long)k);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_cand == 0 || k == 0) {
        if (hipMemsetAsync(n_picked, 0, sizeof(int64_t), s) != hipSuccess) {
            set_error("%s: hipMemsetAsync of n_picked failed", what);
            return TCR_ERR_HIP;
        }
        return TCR_OK;
    }
    TCR_REQUIRE(cand_value && workspace && picked, "%s: null argument", what);
    TCR_TRY(mine_ws_check(what, n_cand, true, ws_bytes));
    const MineWs w = mine_ws(workspace, n_cand, true);
    if (hipMemsetAsync(w.hist, 0, (4 * 256 + 64) * sizeof(unsigned), s) != hipSuccess) {
        set_error("%s: hipMemsetAsync of the histograms failed", what);
        return TCR_ERR_HIP;
    }
    MinePickArgs a{};
    a.value = cand_value; a.kind = cand_kind; a.bits = w.bits; a.prefix = w.prefix; a.hist = w.hist; a.state = w.hist + 4 * 256;
    a.n = n_cand; a.kind_mask = kind_mask; a.k = (unsigned)std::min<int64_t>(k, n_cand);
    const unsigned hist_blocks = (unsigned)ceil_div64(n_cand, 256 * kMineItems), blocks = (unsigned)ceil_div64(n_cand, 256);
    for (a.pass = 0; a.pass < 4; ++a.pass) {
        hipLaunchKernelGGL(mine_hist_kernel, dim3(hist_blocks), dim3(256), 0, s, a);
        TCR_TRY(check_launch("mine_hist_kernel"));
        hipLaunchKernelGGL(mine_digit_kernel, dim3(1), dim3(256), 0, s, a);
        TCR_TRY(check_launch("mine_digit_kernel"));
    }
    hipLaunchKernelGGL(mine_pick_kernel<true>, dim3(blocks), dim3(256), 0, s, a);
    TCR_TRY(check_launch("mine_pick_kernel"));
    SelectArgs sa = mine_select_args(w, n_cand, picked, nullptr);
    TCR_TRY(mine_count_scan(sa, s));
    hipLaunchKernelGGL(select_prefix_kernel, dim3(sa.tiles), dim3(256), 0, s, sa);
    TCR_TRY(check_launch("select_prefix_kernel"));
    hipLaunchKernelGGL(mine_pick_kernel<false>, dim3(blocks), dim3(256), 0, s, a);
    TCR_TRY(check_launch("mine_pick_kernel"));
    sa.n_selected = n_picked;
    TCR_TRY(mine_count_scan(sa, s));
    hipLaunchKernelGGL(select_compact_kernel, dim3(sa.tiles), dim3(256), 0, s, sa);
    return check_launch("select_compact_kernel");
}

extern "C" int tcr_mine_gather(int n_signals, const int64_t* sample_offsets, const float* samples, int64_t n_clips, const int32_t* clip_signal,
                               const int64_t* clip_first, int n_samples, float* out, int16_t* out_pcm, void* stream) {
    const char* what = "tcr_mine_gather";
    TCR_REQUIRE(out || out_pcm, "%s: out and out_pcm are both null", what);
    TCR_REQUIRE(n_signals > 0, "%s: the number of signals must be positive (got %d)", what, n_signals);
    TCR_REQUIRE(n_samples > 0, "%s: n_samples must be positive (got %d)", what, n_samples);
    TCR_REQUIRE(n_clips >= 0, "%s: n_clips must be >= 0 (got %lld)", what, (long long)n_clips);
    if (n_clips == 0) return TCR_OK;
    TCR_REQUIRE(sample_offsets && samples && clip_signal && clip_first, "%s: null argument", what);
    MineGatherArgs a{};
    a.samples = samples; a.sample_off = sample_offsets; a.clip_signal = clip_signal; a.clip_first = clip_first; a.out = out; a.out_pcm = out_pcm;
    a.n_samples = n_samples; a.N = n_signals;
    a.parts = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(n_samples, 4 * 256 * 4), 64));      // four 16-byte stores per thread
    TCR_REQUIRE(n_clips * a.parts < ((int64_t)1 << 31), "%s: %lld clips of %d samples are too many for one launch", what, (long long)n_clips,
                n_samples);
    hipLaunchKernelGGL(mine_gather_kernel, dim3((unsigned)(n_clips * a.parts)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("mine_gather_kernel");
}
