// Many streaming steps in one call (tcr_stream_scan): tcr_scan's chunks, started from a stream state (stream.hip) and written back
// to it, so that the call is bitwise m calls of tcr_stream_step -- outputs and state.
//
// In frames of  x = tail ++ samples  (the stream's tail, zeros after a reset, then the call's L = m k hop samples), new frame j >= 0
// covers x[j hop, j hop + win): the samples tcr_stream_step's staging rows hold for the same frame, so the frame is bitwise the
// streaming one (a frame is a pure function of its samples).  Column t of step i's window is new frame (i + 1) k - T + t; a negative
// index -e is column T - e of the carried window (the zero window after a reset).
//
// Group g of a stream is one front-end row of F = G k + T - k frames from new frame g G k + k - T on: tcr_scan's rows, with the
// carried window in place of its silent prefix.  Frames of negative index are computed from zeros and never gathered.  Per chunk:
//   stream_scan_stage_kernel   the staging rows (tail ++ samples, zeros outside);
//   frontend_pk3_kernel        <.., STREAM = true>, as in tcr_scan;
//   stream_scan_gather_kernel  the planar windows: frame-row columns, or carried columns for negative frames (2-D graph:
//                              stream_scan_gather_plane_kernel writes the same values as its planes);
//   stream_scan_carry_kernel   window and tail write-back of the streams whose last group is in this chunk (their last step's
//                              window, gathered just before; the last tail_len samples of x, the old tail read before it is written);
//                              a stream's groups are consecutive, so no later chunk reads its window or tail (2-D graph:
//                              stream_scan_carry_plane_kernel, the planar state window read back from the plane);
//   the network (detect_model.h), scan_scatter_kernel (tcr_scan's).
// Once per call:
//   stream_scan_smooth_kernel    scan_smooth_kernel with the ring in front: count_i = min(count0 + i + 1, W), the vectors of steps
//                                before the call from ring slots (head0 - d) mod W, oldest first, through smooth_mean;
//   stream_scan_suppress_kernel  the ring write-back (the last min(W, m) vectors at slots (head0 + i) mod W: the smoothing has read
//                                the old ones), suppress_walk from the carried prev_label and prev_step - n0 (int64, may be
//                                negative), then the five detector integers.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after scan.hip).
#pragma once
#include <algorithm>

#include "frontend_plan.h"
#include "frontend_args.h"

namespace tcr {

struct StreamScanStageArgs {
    const float* samples;       // [S][L]
    const uint8_t* reset;       // [S] or null
    const float* tail;          // [S][tail_len]
    float* stage;               // [R][stride]
    int64_t L, stride, q0, rows, groups, step_hop, first;  // step_hop = G k hop; first = (k - T) hop: group 0's first position in x
    int tail_len;
};

// Staging row r = group q0 + r (stream q / groups, group q % groups): x from position g G k hop + (k - T) hop on, zeros outside x.
// One thread per staged sample.
__global__ __launch_bounds__(256) void stream_scan_stage_kernel(const StreamScanStageArgs a) {
    const int64_t total = a.rows * a.stride;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / a.stride, x = e - r * a.stride;
        const int64_t q = a.q0 + r, n = q / a.groups, g = q - n * a.groups;
        const int64_t pos = g * a.step_hop + a.first + x;                      // position in x = tail ++ samples
        float v = 0.f;
        if (pos >= a.tail_len) {
            if (pos - a.tail_len < a.L) v = a.samples[n * a.L + pos - a.tail_len];
        } else if (pos >= 0 && !(a.reset && a.reset[n])) {
            v = a.tail[n * a.tail_len + pos];
        }
        a.stage[e] = v;
    }
}

struct StreamScanGatherArgs {
    const float* frames;        // [R][n_coef][F + 2 kHalo]
    float* windows;             // [R G][n_coef][tp]
    const float* window;        // the state's windows [S][n_coef][tp]
    const float* zw;            // the zero window [n_coef][tp]
    const uint8_t* reset;       // [S] or null
    int64_t q0, groups;
    int G, k, T, tp, n_coef, ftp;
};

// One workgroup per window slot b = r G + j (step i = g G + j): column t is column j k + t of frame row r when new frame
// (i + 1) k - T + t >= 0, else column (i + 1) k + t of the carried window; the halo is zero.
__global__ __launch_bounds__(256) void stream_scan_gather_kernel(const StreamScanGatherArgs a) {
    const int b = blockIdx.x;
    const int r = b / a.G, j = b - r * a.G;
    const int64_t q = a.q0 + r, s = q / a.groups, g = q - s * a.groups;
    const int64_t i1 = (g * a.G + j + 1) * a.k;                                 // (i + 1) k
    const int sh = i1 < a.T ? (int)i1 : a.T;                                    // carried columns: t < T - sh
    const float* src = a.frames + (size_t)r * a.n_coef * a.ftp + j * a.k;      // window column x <- frame-row column j k + x
    const float* old = (a.reset && a.reset[s] ? a.zw : a.window + (size_t)s * a.n_coef * a.tp) + sh;
    float* dst = a.windows + (size_t)b * a.n_coef * a.tp;
    const int n = a.n_coef * a.tp;
    const int dc = 256 / a.tp, dx = 256 - dc * a.tp;
    int c = threadIdx.x / a.tp, x = threadIdx.x - c * a.tp;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int t = x - kHalo;
        dst[i] = t >= 0 && t < a.T ? (t + sh < a.T ? old[c * a.tp + x] : src[(size_t)c * a.ftp + x]) : 0.f;
        c += dc;
        x += dx;
        if (x >= a.tp) { x -= a.tp; ++c; }
    }
}

// stream_scan_gather_kernel for a 2-D graph: slot b's window as its [T x n_coef] plane, written in plane order: plane offset
// t n_coef + c <- window column t, coefficient c (features_to_plane_kernel's map, net2d_kernels.hip), zero halo.  A pure copy:
// bitwise stream_scan_gather_kernel followed by features_to_plane_kernel.
__global__ __launch_bounds__(256) void stream_scan_gather_plane_kernel(const StreamScanGatherArgs a) {
    const int b = blockIdx.x;
    const int r = b / a.G, j = b - r * a.G;
    const int64_t q = a.q0 + r, s = q / a.groups, g = q - s * a.groups;
    const int64_t i1 = (g * a.G + j + 1) * a.k;                                 // (i + 1) k
    const int sh = i1 < a.T ? (int)i1 : a.T;                                    // carried columns: t < T - sh
    const float* src = a.frames + (size_t)r * a.n_coef * a.ftp + j * a.k;      // window column x <- frame-row column j k + x
    const float* old = (a.reset && a.reset[s] ? a.zw : a.window + (size_t)s * a.n_coef * a.tp) + sh;
    const int n = a.T * a.n_coef, pp = n + 2 * kHalo;
    float* dst = a.windows + (size_t)b * pp;
    for (int i = threadIdx.x; i < pp; i += 256) {
        const int o = i - kHalo;
        float v = 0.f;
        if (o >= 0 && o < n) {
            const int t = o / a.n_coef, c = o - t * a.n_coef, x = t + kHalo;
            v = t + sh < a.T ? old[c * a.tp + x] : src[(size_t)c * a.ftp + x];
        }
        dst[i] = v;
    }
}

struct StreamScanCarryArgs {
    const float* windows;       // the chunk's [R G][n_coef][tp]
    const float* samples;       // [S][L]
    const uint8_t* reset;       // [S] or null
    float* window;              // the state's [S][n_coef][tp]
    float* tail;                // [S][tail_len]
    int64_t L, q0, groups, steps, s0;
    int G, win_elems, tail_len;
};

// One workgroup per stream s0 + blockIdx.x whose last group is in the chunk: window = its last step's gathered window (planar, zero
// halo: the state's layout); tail = the last tail_len samples of  tail ++ samples  (old samples that survive a short call are read
// into LDS before the tail is written).
__global__ __launch_bounds__(256) void stream_scan_carry_kernel(const StreamScanCarryArgs a) {
    __shared__ float s_tail[kMaxTail];
    const int64_t s = a.s0 + blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t b = (s * a.groups + a.groups - 1 - a.q0) * a.G + a.steps - 1 - (a.groups - 1) * a.G;
    const float* wsrc = a.windows + b * a.win_elems;
    float* wdst = a.window + s * a.win_elems;
    for (int i = tid; i < a.win_elems; i += 256) wdst[i] = wsrc[i];
    const bool rst = a.reset && a.reset[s];
    float* tail = a.tail + s * a.tail_len;
    const float* src = a.samples + s * a.L;
    const int keep = a.L < a.tail_len ? (int)(a.tail_len - a.L) : 0;          // old tail samples L .. tail_len - 1 stay
    for (int i = tid; i < keep; i += 256) s_tail[i] = rst ? 0.f : tail[a.L + i];
    __syncthreads();
    for (int i = tid; i < a.tail_len; i += 256) tail[i] = i < keep ? s_tail[i] : src[a.L - a.tail_len + i];
}

struct StreamScanCarryPlaneArgs {
    StreamScanCarryArgs c;      // c.win_elems: the state's n_coef tp floats per stream
    int T, n_coef, tp;
};

// stream_scan_carry_kernel for a 2-D graph: the chunk's windows are planes [R G][T n_coef + 2 TCR_HALO]; the state's planar window
// is read back from the last step's plane (column t, coefficient c <- plane offset t n_coef + c; zero halo).  The tail as there.
__global__ __launch_bounds__(256) void stream_scan_carry_plane_kernel(const StreamScanCarryPlaneArgs p) {
    __shared__ float s_tail[kMaxTail];
    const StreamScanCarryArgs& a = p.c;
    const int64_t s = a.s0 + blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t b = (s * a.groups + a.groups - 1 - a.q0) * a.G + a.steps - 1 - (a.groups - 1) * a.G;
    const int pp = p.T * p.n_coef + 2 * kHalo;
    const float* wsrc = a.windows + b * pp + kHalo;
    float* wdst = a.window + s * a.win_elems;
    for (int i = tid; i < a.win_elems; i += 256) {
        const int c = i / p.tp, t = i - c * p.tp - kHalo;
        wdst[i] = t >= 0 && t < p.T ? wsrc[t * p.n_coef + c] : 0.f;
    }
    const bool rst = a.reset && a.reset[s];
    float* tail = a.tail + s * a.tail_len;
    const float* src = a.samples + s * a.L;
    const int keep = a.L < a.tail_len ? (int)(a.tail_len - a.L) : 0;          // old tail samples L .. tail_len - 1 stay
    for (int i = tid; i < keep; i += 256) s_tail[i] = rst ? 0.f : tail[a.L + i];
    __syncthreads();
    for (int i = tid; i < a.tail_len; i += 256) tail[i] = i < keep ? s_tail[i] : src[a.L - a.tail_len + i];
}

struct StreamScanSmoothArgs {
    const float* probs;         // [S][steps][C]
    const float* ring;          // [W][S][C]
    const int* ist;             // [5][S]
    const uint8_t* reset;       // [S] or null
    float* smoothed;
    int32_t* top;               // [S][steps]
    float* score;
    int32_t* is_new;            // here: the candidate flag, top + 1 (candidate) or 0
    int64_t windows, steps;
    int S, C, W, min_count;
    float threshold;
};

// scan_smooth_kernel's lanes, with the detector's ring in front of the call's probabilities: step i averages the last
// count = min(count0 + i + 1, W) vectors, those of steps before the call from ring slot (head0 + j) mod W (j < 0, oldest first).
__global__ __launch_bounds__(256) void stream_scan_smooth_kernel(const StreamScanSmoothArgs a) {
    __shared__ float s_sm[256];
    const int C = a.C, W = a.W;
    const int per = 256 / C;
    const int ls = threadIdx.x / C, c = threadIdx.x - ls * C;
    const int64_t w = (int64_t)blockIdx.x * per + ls;                   // window = s steps + i
    const bool live = ls < per && w < a.windows;
    int count = 0;
    if (live) {
        const int64_t s = w / a.steps, i = w - s * a.steps;
        const bool rst = a.reset && a.reset[s];
        const int head0 = rst ? 0 : a.ist[s], count0 = rst ? 0 : a.ist[a.S + s];
        count = count0 + i + 1 < W ? (int)(count0 + i + 1) : W;
        int64_t jj = i - count + 1;                                     // oldest step (< 0: before the call)
        int slot = jj < 0 ? (head0 + (int)jj < 0 ? head0 + (int)jj + W : head0 + (int)jj) : 0;
        const float* p = a.probs + s * a.steps * C + c;
        const size_t ring_row = (size_t)a.S * C, sc = (size_t)s * C + c;
        const float v = smooth_mean(count, [&]() {
            float x;
            if (jj < 0) {
                x = a.ring[slot * ring_row + sc];
                slot = slot + 1 == W ? 0 : slot + 1;
            } else {
                x = p[jj * C];
            }
            ++jj;
            return x;
        });
        a.smoothed[w * C + c] = v;
        s_sm[threadIdx.x] = v;
    }
    __syncthreads();
    if (!live || c != 0) return;
    int best = 0;
    float best_v = s_sm[threadIdx.x];
    for (int cc = 1; cc < C; ++cc) {
        const float v = s_sm[threadIdx.x + cc];
        if (v > best_v) { best = cc; best_v = v; }
    }
    const bool warm = count >= a.min_count;
    a.top[w] = warm ? best : -1;
    a.score[w] = warm ? best_v : 0.f;
    a.is_new[w] = warm && best_v > a.threshold ? best + 1 : 0;
}

// scan_suppress_kernel's walk (scan.hip) over one stream's flags fl[0 .. steps), from (prev_label, prev_step) instead of (-1, 0); wave 0
// ends with the final state.  s_val / s_any: the caller's LDS, 256 x kSuppressPer and 2 ints.  (The same statements: as a function
// shared with scan_suppress_kernel it changes that kernel's instruction schedule, so the kernel keeps its own copy.)
__device__ __forceinline__ void suppress_walk(int32_t* fl, int64_t steps, int suppression, int& prev_label, int64_t& prev_step,
                                              int* s_val, int* s_any) {
    constexpr int PASS = 256 * kSuppressPer;
    constexpr int NONE = 0x7fffffff;
    const int tid = threadIdx.x;
    if (tid == 0) s_any[0] = 0;
    __syncthreads();
    int it = 0;
    for (int64_t base = 0; base < steps; base += PASS, ++it) {
        int v[kSuppressPer];
#pragma unroll
        for (int e = 0; e < kSuppressPer; ++e) {
            const int64_t idx = base + e * 256 + tid;
            v[e] = idx < steps ? fl[idx] : 0;
        }
        bool any = false;
#pragma unroll
        for (int e = 0; e < kSuppressPer; ++e) {
            s_val[e * 256 + tid] = v[e];
            any |= v[e] != 0;
        }
        if (tid == 0) s_any[(it + 1) & 1] = 0;         // (the other slot: read by every thread behind the previous pass's barrier)
        if (any) s_any[it & 1] = 1;
        __syncthreads();
        if (s_any[it & 1] == 0) continue;
        if (tid < 64) {
            const int n = (int)(steps - base < PASS ? steps - base : PASS);
            int cur = 0;
            while (cur < n) {
                if (prev_label != -1) {
                    const int64_t lo = prev_step + suppression + 1 - base;
                    if (lo > cur) cur = lo < n ? (int)lo : n;
                    if (cur >= n) break;
                }
                int key = NONE;                                 // step offset << 8 | label of the lowest candidate that fires
#pragma unroll
                for (int u = 3; u >= 0; --u) {
                    const int j = cur + u * 64 + tid;
                    const int val = j < n ? s_val[j] : 0;
                    if (val != 0 && val - 1 != prev_label) key = j << 8 | (val - 1);
                }
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) key = min(key, __shfl_xor(key, m));
                if (key == NONE) { cur += 256; continue; }
                const int first = key >> 8;
                prev_label = key & 255;
                prev_step = base + first;
                if (tid == 0) s_val[first] = -1;
                cur = first + 1;
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kSuppressPer; ++e) {
            const int64_t idx = base + e * 256 + tid;
            if (v[e] != 0) fl[idx] = s_val[e * 256 + tid] == -1 ? 1 : 0;
        }
    }
}

struct StreamScanSuppressArgs {
    const float* probs;         // [S][steps][C]
    int32_t* is_new;            // [S][steps], candidate flags in, detections out
    float* ring;                // [W][S][C]
    int* ist;                   // [5][S]
    const uint8_t* reset;       // [S] or null
    int64_t steps;
    int S, C, W, suppression;
};

// One workgroup per stream: the ring write-back, scan_suppress_kernel's walk from the carried detector, the detector integers.
__global__ __launch_bounds__(256) void stream_scan_suppress_kernel(const StreamScanSuppressArgs a) {
    __shared__ int s_val[256 * kSuppressPer];
    __shared__ int s_any[2];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int S = a.S, C = a.C, W = a.W;
    const bool rst = a.reset && a.reset[s];
    const int head0 = rst ? 0 : a.ist[s], count0 = rst ? 0 : a.ist[S + s];
    const int n0 = rst ? 0 : a.ist[4 * S + s];
    int prev_label = rst ? -1 : a.ist[2 * S + s];                      // (wave 0's, the same in its lanes)
    int64_t prev_step = rst ? 0 : (int64_t)a.ist[3 * S + s] - n0;       // relative to the call's first step
    const int nw = a.steps < W ? (int)a.steps : W;                      // the last nw vectors stay in the ring
    const int64_t i0 = a.steps - nw;
    for (int e = tid; e < nw * C; e += 256) {
        const int d = e / C, c = e - d * C;
        const int slot = (int)((head0 + i0 + d) % W);
        a.ring[(size_t)slot * S * C + (size_t)s * C + c] = a.probs[((int64_t)s * a.steps + i0 + d) * C + c];
    }
    suppress_walk(a.is_new + (int64_t)s * a.steps, a.steps, a.suppression, prev_label, prev_step, s_val, s_any);
    if (tid == 0) {                                                     // (every thread read the integers before the walk's barriers)
        a.ist[s] = (int)((head0 + a.steps) % W);
        a.ist[S + s] = count0 + a.steps < W ? (int)(count0 + a.steps) : W;
        a.ist[2 * S + s] = prev_label;
        a.ist[3 * S + s] = (int)(n0 + prev_step);
        a.ist[4 * S + s] = (int)(n0 + a.steps);
    }
}

namespace {

int stream_scan(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* m, int n_streams, int64_t n_samples, int k,
                const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state, void* workspace, size_t ws_bytes,
                float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream, const char* what) {
    TCR_REQUIRE(plan_dev && m && m->params && m->aux && det && samples && state && workspace && logits && probs && smoothed && top && score &&
                is_new, "%s: null argument", what);
    ModelIO io;
    TCR_TRY(stream_check(cfg, m, n_streams, k, det, what, io));
    const int64_t khop = (int64_t)k * cfg->hop;
    TCR_REQUIRE(n_samples > 0 && n_samples % khop == 0, "%s: the signal length %lld is not a positive multiple of k * hop = %lld", what,
                (long long)n_samples, (long long)khop);
    const int64_t steps = n_samples / khop;
    const StreamGeom sg = stream_geom(*cfg, *m, io, n_streams, k, det->average_steps);
    TCR_REQUIRE((int64_t)n_streams * steps * sg.classes < ((int64_t)1 << 31),
                "%s: %d streams x %lld steps is too large", what, n_streams, (long long)steps);
    ScanGeom g;
    TCR_TRY(scan_chunking(*cfg, *m, io, k, steps, n_streams, ws_bytes, what, g));
    const int G = g.G;
    const int64_t groups = ceil_div64(steps, G), total_groups = groups * n_streams;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* st = static_cast<float*>(state);
    float* ws = static_cast<float*>(workspace);
    int* ist = reinterpret_cast<int*>(st + sg.ist_off);
    const int ftp = tcr_padded_len(g.F);
    for (int64_t q0 = 0; q0 < total_groups; q0 += g.R) {
        const int rows = (int)std::min<int64_t>(g.R, total_groups - q0);
        const int slots = rows * G;
        StreamScanStageArgs sa;
        sa.samples = samples; sa.reset = reset; sa.tail = st + sg.tail_off; sa.stage = ws + g.stage_off; sa.L = n_samples;
        sa.stride = g.stage_stride; sa.q0 = q0; sa.rows = rows; sa.groups = groups; sa.step_hop = (int64_t)G * khop;
        sa.first = (int64_t)(k - g.T) * cfg->hop; sa.tail_len = sg.tail_len;
        const int64_t staged = (int64_t)rows * g.stage_stride;
        hipLaunchKernelGGL(stream_scan_stage_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(staged, 256), 8 * (int64_t)device_cus())), dim3(256),
                           0, s, sa);
        TCR_TRY(check_launch("stream_scan_stage_kernel"));
        TCR_TRY(stream_frontend(*cfg, plan_dev, ws + g.stage_off, g.stage_stride, rows, g.F, ws + g.frames_off, s, ftp));
        StreamScanGatherArgs ga;
        ga.frames = ws + g.frames_off; ga.windows = ws + g.win_off; ga.window = st + sg.win_off; ga.zw = st + sg.zw_off; ga.reset = reset;
        ga.q0 = q0; ga.groups = groups; ga.G = G; ga.k = k; ga.T = g.T; ga.tp = g.tp; ga.n_coef = g.n_coef; ga.ftp = ftp;
        if (g.planes) {
            hipLaunchKernelGGL(stream_scan_gather_plane_kernel, dim3(slots), dim3(256), 0, s, ga);
            TCR_TRY(check_launch("stream_scan_gather_plane_kernel"));
        } else {
            hipLaunchKernelGGL(stream_scan_gather_kernel, dim3(slots), dim3(256), 0, s, ga);
            TCR_TRY(check_launch("stream_scan_gather_kernel"));
        }
        // the streams whose last group (s groups + groups - 1) is one of this chunk's rows
        const int64_t s_lo = (q0 + 1 + groups - 1) / groups - 1, s_hi = (q0 + rows) / groups - 1;
        if (s_hi >= s_lo) {
            StreamScanCarryArgs ca;
            ca.windows = ws + g.win_off; ca.samples = samples; ca.reset = reset; ca.window = st + sg.win_off; ca.tail = st + sg.tail_off;
            ca.L = n_samples; ca.q0 = q0; ca.groups = groups; ca.steps = steps; ca.s0 = s_lo; ca.G = G; ca.win_elems = g.n_coef * g.tp;
            ca.tail_len = sg.tail_len;
            if (g.planes) {
                StreamScanCarryPlaneArgs pa;
                pa.c = ca; pa.T = g.T; pa.n_coef = g.n_coef; pa.tp = g.tp;
                hipLaunchKernelGGL(stream_scan_carry_plane_kernel, dim3((unsigned)(s_hi - s_lo + 1)), dim3(256), 0, s, pa);
                TCR_TRY(check_launch("stream_scan_carry_plane_kernel"));
            } else {
                hipLaunchKernelGGL(stream_scan_carry_kernel, dim3((unsigned)(s_hi - s_lo + 1)), dim3(256), 0, s, ca);
                TCR_TRY(check_launch("stream_scan_carry_kernel"));
            }
        }
        TCR_TRY(model_forward(*m, ws + g.win_off, slots, ws + g.net_off, ws_bytes - (size_t)g.net_off * sizeof(float), ws + g.logits_off,
                              ws + g.probs_off, stream));
        ScanScatterArgs xa;
        xa.logits_in = ws + g.logits_off; xa.probs_in = ws + g.probs_off; xa.logits = logits; xa.probs = probs; xa.q0 = q0;
        xa.groups = groups; xa.steps = steps; xa.G = G; xa.C = g.classes; xa.slots = slots;
        hipLaunchKernelGGL(scan_scatter_kernel, dim3(ceil_div(slots * g.classes, 256)), dim3(256), 0, s, xa);
        TCR_TRY(check_launch("scan_scatter_kernel"));
    }
    StreamScanSmoothArgs ma;
    ma.probs = probs; ma.ring = st + sg.ring_off; ma.ist = ist; ma.reset = reset; ma.smoothed = smoothed; ma.top = top; ma.score = score;
    ma.is_new = is_new; ma.windows = (int64_t)n_streams * steps; ma.steps = steps; ma.S = n_streams; ma.C = g.classes; ma.W = det->average_steps;
    ma.min_count = det->min_count; ma.threshold = det->threshold;
    hipLaunchKernelGGL(stream_scan_smooth_kernel, dim3((unsigned)ceil_div64(ma.windows, 256 / g.classes)), dim3(256), 0, s, ma);
    TCR_TRY(check_launch("stream_scan_smooth_kernel"));
    StreamScanSuppressArgs pa;
    pa.probs = probs; pa.is_new = is_new; pa.ring = st + sg.ring_off; pa.ist = ist; pa.reset = reset; pa.steps = steps; pa.S = n_streams;
    pa.C = g.classes; pa.W = det->average_steps; pa.suppression = det->suppression_steps;
    hipLaunchKernelGGL(stream_scan_suppress_kernel, dim3(n_streams), dim3(256), 0, s, pa);
    return check_launch("stream_scan_suppress_kernel");
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_stream_scan(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                               const float* frozen_ss, int n_streams, int64_t n_samples, int k, const tcr_detect_cfg* det,
                               const float* samples, const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, float* logits,
                               float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    const tcr_model_ref m = tcresnet_ref(net, params, frozen_ss);
    return stream_scan(cfg, plan_dev, &m, n_streams, n_samples, k, det, samples, reset, state, workspace, ws_bytes, logits, probs, smoothed,
                       top, score, is_new, stream, "tcr_stream_scan");
}

extern "C" int tcr_stream_scan_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams,
                                 int64_t n_samples, int k, const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state,
                                 void* workspace, size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score,
                                 int32_t* is_new, void* stream) {
    return stream_scan(cfg, plan_dev, model, n_streams, n_samples, k, det, samples, reset, state, workspace, ws_bytes, logits, probs,
                       smoothed, top, score, is_new, stream, "tcr_stream_scan_m");
}
