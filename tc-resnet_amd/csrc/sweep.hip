// Detection sweeps (tcr_detect_sweep): the streaming detector's suppression rule (tcr_stream_step) run for T thresholds at once over
// the top / score a scan (or stacked streaming pushes) produced, with the detections scored against labelled keyword events.
//
// Only the rule's last stage depends on the threshold: top and score do not.  The rule is sequential and keeps state (prev_label,
// prev_step), so it is walked once per (signal, threshold), but the walks share their input:
//   sweep_kernel  a workgroup per (signal, block of kSweepBlockT thresholds) stages passes of kSweepPass steps into LDS once --
//                 the candidate score (score where 0 <= top < C, NaN elsewhere: NaN > t is false for every t, so such a step never
//                 fires), the label, and per step the signal's event that covers it (index and label, -1 where none) -- and each
//                 wave walks kSweepWaveT thresholds over the staged pass, one after the other, with scan_suppress_kernel's walk:
//                 after a detection it jumps past the suppressed steps, then probes 256 steps at a time (four per lane, the lowest
//                 step by a wave minimum) for the first candidate whose label differs from prev_label.  A threshold at or
//                 above the pass's largest candidate score skips the pass: non-candidates never fire or change the state.
// A detection (step i, label c) is counted in LDS by lane 0 of its wave: detections[c] always; when event e covers i and has label
// c, hits[c] if e is not the event the threshold's last hit went to, duplicates[c] if it is (events are sorted and disjoint and the
// walk goes in step order, so every earlier detection inside e came right before).  The counters are written out at the end.
// `fired` (optional) is zeroed by a memset and gets a byte store per detection.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after scan.hip).
#pragma once
#include <algorithm>
#include <climits>

namespace tcr {

namespace {

constexpr int kSweepPer = 8;                            // steps per thread and pass (256 x 8 = 2048 steps a pass: 21 KB of LDS,
                                                        // seven workgroups per CU -- the walks are latency-bound)
constexpr int kSweepPass = 256 * kSweepPer;
constexpr int kSweepWaveT = 4;                          // thresholds per wave
constexpr int kSweepBlockT = 4 * kSweepWaveT;           // thresholds per workgroup (wave w walks t0 + w, t0 + w + 4, ...)
constexpr int kSweepMaxClasses = 256;                   // labels are packed into 8 bits of the probe's key

// Minimum over the wave, in every lane: the row16_sum pattern (tcr_common.h: quad xor 1, quad xor 2, row_half_mirror, row_mirror
// as DPP operands on the VALU), then xor 16 and xor 32 through bpermutes -- two LDS-pipe round trips per probe instead of six.
__device__ __forceinline__ int wave_min(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true));      // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true));     // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true));     // row_mirror
    v = min(v, __shfl_xor(v, 16));
    return min(v, __shfl_xor(v, 32));
}

}  // namespace

struct SweepArgs {
    const int32_t* top;         // [N][steps]
    const float* score;
    const int64_t* valid_steps; // [N] or null
    const float* thresholds;    // [T]
    const int32_t* ev_off;      // [N + 1] or null
    const int64_t* ev_first;
    const int64_t* ev_last;
    const int32_t* ev_label;
    int32_t* detections;        // [N][T][C]
    int32_t* hits;              // [N][T][C] or null
    int32_t* duplicates;
    uint8_t* fired;             // [T][N][steps] or null (zeroed before the launch)
    int64_t steps;
    int n_signals, n_thr, C, suppression, tblocks;
    const int64_t* step_off;    // ragged (tcr_detect_sweep_ragged): [N + 1]; top / score are packed, fired is [T][step_off[N]]
};

// Dynamic LDS: counters [3][kSweepBlockT][C] (detections, hits, duplicates).  At most 80 VGPRs: six waves per SIMD (86 unbounded: five;
// 72 for seven spills).  RAGGED: the signal's rows and its step count come from step_off, on the device, and the workgroup zeroes
// its thresholds' rows of `fired` itself before it walks (the host does not know their total).
template <bool RAGGED>
__global__ __launch_bounds__(256, 6) void sweep_kernel(const SweepArgs a) {
    constexpr int NONE = 0x7fffffff;
    __shared__ float s_sc[kSweepPass];                  // candidate score (NaN: never fires)
    __shared__ uint8_t s_top[kSweepPass];               // label
    __shared__ int s_ev[kSweepPass];                    // covering event (index within the signal) or -1
    __shared__ uint8_t s_evl[kSweepPass];               // its label (0 .. C - 1)
    __shared__ float s_wmax[4];
    __shared__ int s_red[2][4];
    int* cnt = reinterpret_cast<int*>(dyn_lds());
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int C = a.C;
    const int n = (int)(blockIdx.x / (unsigned)a.tblocks), t0 = (int)(blockIdx.x - (unsigned)n * a.tblocks) * kSweepBlockT;
    const int ncnt = 3 * kSweepBlockT * C;
    for (int i = tid; i < ncnt; i += 256) cnt[i] = 0;
    int64_t vs = a.steps, row0, total = 0;
    if constexpr (RAGGED) {
        row0 = a.step_off[n];
        vs = a.step_off[n + 1] - row0;
        if (vs < 0) vs = 0;
        total = a.step_off[a.n_signals];
        if (a.fired) {
            for (int r = 0; r < kSweepBlockT && t0 + r < a.n_thr; ++r) {
                uint8_t* f = a.fired + (int64_t)(t0 + r) * total + row0;
                for (int64_t i = tid; i < vs; i += 256) f[i] = 0;
            }
        }
    } else {
        row0 = (int64_t)n * a.steps;
        if (a.valid_steps) {
            const int64_t v = a.valid_steps[n];
            vs = v < 0 ? 0 : v < a.steps ? v : a.steps;
        }
    }
    const bool events = a.ev_off != nullptr;
    int64_t e_lo = 0, e_hi = 0, e_base = 0;
    if (events) {
        e_base = a.ev_off[n];
        e_lo = e_base;
        e_hi = a.ev_off[n + 1];
        if (e_hi < e_lo) e_hi = e_lo;
    }
    float thr[kSweepWaveT];
    int prev[kSweepWaveT], last_hit[kSweepWaveT];
    int64_t prev_step[kSweepWaveT];
#pragma unroll
    for (int q = 0; q < kSweepWaveT; ++q) {
        const int t = t0 + wave + 4 * q;
        thr[q] = t < a.n_thr ? a.thresholds[t] : __builtin_nanf("");    // (past T: never fires)
        prev[q] = -1;
        prev_step[q] = 0;
        last_hit[q] = -1;
    }
    const int32_t* top = a.top + row0;
    const float* score = a.score + row0;
    __syncthreads();
    for (int64_t base = 0; base < vs; base += kSweepPass) {
        const int len = (int)(vs - base < kSweepPass ? vs - base : kSweepPass);
        float m = -__builtin_inff();
#pragma unroll
        for (int e = 0; e < kSweepPer; ++e) {
            const int j = e * 256 + tid;
            float sc = __builtin_nanf("");
            int lab = 0;
            if (j < len) {
                const int c = top[base + j];
                if (c >= 0 && c < C) {
                    sc = score[base + j];
                    lab = c;
                }
            }
            s_sc[j] = sc;
            s_top[j] = (uint8_t)lab;
            if (events) s_ev[j] = -1;
            m = fmaxf(m, sc);                           // (NaN ignored)
        }
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) m = fmaxf(m, __shfl_xor(m, k));
        if (lane == 0) s_wmax[wave] = m;
        __syncthreads();
        const float pmax = fmaxf(fmaxf(s_wmax[0], s_wmax[1]), fmaxf(s_wmax[2], s_wmax[3]));
        if (events) {
            // the events that overlap the pass, 256 at a time from the first unfinished one; a thread fills its event's steps.  With
            // sorted disjoint events the finished ones (last < pass end) are a prefix, and an unfinished one ends the search.
            const int64_t pend = base + len;
            for (int it = 0;; ++it) {
                const int64_t e = e_lo + tid;
                int fin = 0;
                if (e < e_hi) {
                    const int64_t f = a.ev_first[e], l = a.ev_last[e];
                    const int lab = a.ev_label[e];
                    if (lab >= 0 && lab < C) {
                        const int64_t lo = f > base ? f : base, hi = l < pend - 1 ? l : pend - 1;
                        for (int64_t s = lo; s <= hi; ++s) {
                            s_ev[s - base] = (int)(e - e_base);
                            s_evl[s - base] = (uint8_t)lab;
                        }
                    }
                    fin = l < pend;
                }
#pragma unroll
                for (int k = 1; k < 64; k <<= 1) fin += __shfl_xor(fin, k);
                if (lane == 0) s_red[it & 1][wave] = fin;
                __syncthreads();
                const int nfin = s_red[it & 1][0] + s_red[it & 1][1] + s_red[it & 1][2] + s_red[it & 1][3];
                e_lo += nfin;
                if (nfin < 256) break;
            }
        }
#pragma unroll
        for (int q = 0; q < kSweepWaveT; ++q) {
            const float th = thr[q];
            if (!(pmax > th)) continue;                 // no candidate in the pass (or t past T)
            int cur = 0;
            while (cur < len) {
                if (prev[q] != -1) {
                    const int64_t lo = prev_step[q] + a.suppression + 1 - base;
                    if (lo > cur) cur = lo < len ? (int)lo : len;
                    if (cur >= len) break;
                }
                int key = NONE;                         // step << 8 | label of the lowest candidate that fires
#pragma unroll
                for (int u = 3; u >= 0; --u) {
                    const int j = cur + u * 64 + lane;
                    if (j < len) {
                        const int lab = s_top[j];
                        if (s_sc[j] > th && lab != prev[q]) key = j << 8 | lab;
                    }
                }
                key = wave_min(key);
                if (key == NONE) { cur += 256; continue; }
                const int first = key >> 8, lab = key & 255;
                prev[q] = lab;
                prev_step[q] = base + first;
                const int ev = events ? s_ev[first] : -1;
                const bool hit = ev >= 0 && s_evl[first] == lab;
                const bool dup = hit && ev == last_hit[q];
                if (hit) last_hit[q] = ev;
                if (lane == 0) {
                    int* row = cnt + (wave + 4 * q) * C + lab;
                    row[0] += 1;
                    if (hit) row[(dup ? 2 : 1) * kSweepBlockT * C] += 1;
                    if (a.fired) {
                        if constexpr (RAGGED) a.fired[(int64_t)(t0 + wave + 4 * q) * total + row0 + base + first] = 1;
                        else a.fired[((int64_t)(t0 + wave + 4 * q) * a.n_signals + n) * a.steps + base + first] = 1;
                    }
                }
                cur = first + 1;
            }
        }
        __syncthreads();                                // (the next pass restages)
    }
    __syncthreads();
    for (int i = tid; i < kSweepBlockT * C; i += 256) {
        const int r = i / C, c = i - r * C, t = t0 + r;
        if (t >= a.n_thr) continue;
        const int64_t o = ((int64_t)n * a.n_thr + t) * C + c;
        a.detections[o] = cnt[i];
        if (a.hits) a.hits[o] = cnt[kSweepBlockT * C + i];
        if (a.duplicates) a.duplicates[o] = cnt[2 * kSweepBlockT * C + i];
    }
}

namespace {

template <bool RAGGED>
int sweep_launch(SweepArgs& a, hipStream_t s, const char* what) {
    a.tblocks = (a.n_thr + kSweepBlockT - 1) / kSweepBlockT;
    const size_t lds = (size_t)3 * kSweepBlockT * a.C * sizeof(int);
    if (lds > 24 * 1024 &&                              // (with the static arrays, past 64 KB of LDS: C > 120)
        hipFuncSetAttribute(reinterpret_cast<const void*>(sweep_kernel<RAGGED>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess) {
        set_error("%s: hipFuncSetAttribute failed", what);
        return TCR_ERR_HIP;
    }
    hipLaunchKernelGGL(sweep_kernel<RAGGED>, dim3((unsigned)((int64_t)a.n_signals * a.tblocks)), dim3(256), lds, s, a);
    return check_launch("sweep_kernel");
}

// The refusals of the two entries, in their order (tcr_detect_grid, detect_grid.hip, applies them to its own arguments too).
int sweep_check(const char* what, bool ragged, int n_signals, int64_t steps, const int64_t* step_offsets, int num_classes, const int32_t* top,
                const float* score, int32_t suppression_steps, int n_thresholds, const float* thresholds, const int32_t* event_offsets,
                const int64_t* event_first, const int64_t* event_last, const int32_t* event_label, const int32_t* detections,
                const int32_t* hits, const int32_t* duplicates) {
    TCR_REQUIRE((!ragged || step_offsets) && top && score && thresholds && detections, "%s: null argument", what);
    TCR_REQUIRE(n_signals > 0, "%s: the number of signals must be positive (got %d)", what, n_signals);
    TCR_REQUIRE(ragged || steps > 0, "%s: the number of steps must be positive (got %lld)", what, (long long)steps);
    TCR_REQUIRE(n_thresholds > 0, "%s: the number of thresholds must be positive (got %d)", what, n_thresholds);
    TCR_REQUIRE(num_classes > 0 && num_classes <= kSweepMaxClasses, "%s: num_classes %d outside 1..%d", what, num_classes, kSweepMaxClasses);
    TCR_REQUIRE(suppression_steps >= 0, "%s: suppression_steps must be >= 0 (got %d)", what, suppression_steps);
    TCR_REQUIRE(!event_offsets || (event_first && event_last && event_label && hits && duplicates),
                "%s: events need event_first, event_last, event_label, hits and duplicates", what);
    const bool results_fit = (int64_t)n_signals * n_thresholds * num_classes < ((int64_t)1 << 31);
    if (ragged) {
        TCR_REQUIRE(results_fit, "%s: %d signals x %d thresholds x %d classes is too large", what, n_signals, n_thresholds, num_classes);
    } else {
        TCR_REQUIRE((int64_t)n_signals * steps < ((int64_t)1 << 31) && results_fit,
                    "%s: %d signals x %lld steps x %d thresholds x %d classes is too large", what, n_signals, (long long)steps, n_thresholds,
                    num_classes);
    }
    return TCR_OK;
}

// What the two entries share: the checks, the argument fill and the launch.  Dense: `steps` per signal (checked, and `fired` is
// cleared here); ragged (step_offsets non-null where the entry requires it): the packed rows of step_offsets.
int sweep(const char* what, bool ragged, int n_signals, int64_t steps, const int64_t* step_offsets, int num_classes, const int32_t* top,
          const float* score, const int64_t* valid_steps, int32_t suppression_steps, int n_thresholds, const float* thresholds,
          const int32_t* event_offsets, const int64_t* event_first, const int64_t* event_last, const int32_t* event_label,
          int32_t* detections, int32_t* hits, int32_t* duplicates, uint8_t* fired, void* stream) {
    TCR_TRY(sweep_check(what, ragged, n_signals, steps, step_offsets, num_classes, top, score, suppression_steps, n_thresholds, thresholds,
                        event_offsets, event_first, event_last, event_label, detections, hits, duplicates));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!ragged && fired && hipMemsetAsync(fired, 0, (size_t)n_thresholds * n_signals * steps, s) != hipSuccess) {
        set_error("%s: hipMemsetAsync of fired failed", what);
        return TCR_ERR_HIP;
    }
    SweepArgs a;
    a.top = top; a.score = score; a.valid_steps = valid_steps; a.thresholds = thresholds;
    a.ev_off = event_offsets; a.ev_first = event_first; a.ev_last = event_last; a.ev_label = event_label;
    a.detections = detections; a.hits = hits; a.duplicates = duplicates; a.fired = fired;
    a.steps = steps; a.n_signals = n_signals; a.n_thr = n_thresholds; a.C = num_classes; a.suppression = suppression_steps;
    a.step_off = step_offsets;
    return ragged ? sweep_launch<true>(a, s, what) : sweep_launch<false>(a, s, what);
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_detect_sweep(int n_signals, int64_t steps, int num_classes, const int32_t* top, const float* score,
                                const int64_t* valid_steps, int32_t suppression_steps, int n_thresholds, const float* thresholds,
                                const int32_t* event_offsets, const int64_t* event_first, const int64_t* event_last,
                                const int32_t* event_label, int32_t* detections, int32_t* hits, int32_t* duplicates, uint8_t* fired,
                                void* stream) {
    return sweep("tcr_detect_sweep", false, n_signals, steps, nullptr, num_classes, top, score, valid_steps, suppression_steps, n_thresholds,
                 thresholds, event_offsets, event_first, event_last, event_label, detections, hits, duplicates, fired, stream);
}

extern "C" int tcr_detect_sweep_ragged(int n_signals, const int64_t* step_offsets, int num_classes, const int32_t* top, const float* score,
                                       int32_t suppression_steps, int n_thresholds, const float* thresholds, const int32_t* event_offsets,
                                       const int64_t* event_first, const int64_t* event_last, const int32_t* event_label,
                                       int32_t* detections, int32_t* hits, int32_t* duplicates, uint8_t* fired, void* stream) {
    return sweep("tcr_detect_sweep_ragged", true, n_signals, 0, step_offsets, num_classes, top, score, nullptr, suppression_steps, n_thresholds,
                 thresholds, event_offsets, event_first, event_last, event_label, detections, hits, duplicates, fired, stream);
}
