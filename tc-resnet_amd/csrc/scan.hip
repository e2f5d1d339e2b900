// Offline keyword scanning of long recordings (tcr_scan): every step of N signals in one call, bitwise what a fresh streaming
// detector (stream.hip) returns push by push.
//
// In frames of a signal with n_samples zeros in front (frame f covers padded samples [f hop, f hop + win)), the window of step i is
// frames [(i + 1) k, (i + 1) k + T): tcr_stream_step's window after i + 1 pushes.  A frame is a pure function of its samples
// (frontend_pk3.hip), the network's result for a window does not depend on its batch (DESIGN, net_small_tc8_kernel), the smoothing of
// step i reads the probabilities of steps i - W + 1 .. i only, and the suppression state changes only at candidate steps
// (count >= min_count && score > threshold).  So the windows are computed at the network's batch throughput and only the
// suppression is sequential.
//
// Steps are cut into groups of G consecutive steps of one signal; group g of signal n is one front-end row of F = G k + T - k frames
// starting at frame (g G + 1) k.  A chunk is R consecutive groups (flattened over signals) = R G window slots:
//   scan_stage_kernel     the R staging rows (zero prefix ++ signal, zeros past its end);
//   frontend_pk3_kernel   <.., STREAM = true> over R rows of F frames into frame rows [R][n_coef][F + 2 TCR_HALO] (column 0 on);
//   scan_gather_kernel    the planar windows [R G][n_coef][T + 2 TCR_HALO] (zero halo) from the frame rows; for a 2-D graph
//                         scan_gather_plane_kernel writes its [R G][1][T n_coef + 2 TCR_HALO] planes from them instead;
//   the network at batch R G (detect_model.h: tcr_net_forward_frozen, tcr_dscnn_forward_infer or tcr_g2d_forward_infer, unchanged);
//   scan_scatter_kernel   logits / probs of the slots that are steps (g G + j < steps) into the caller's [N][steps][C].
// Slots past a signal's last step (the last group of a signal may be short) are computed and dropped.  Then, once per call:
//   scan_smooth_kernel    a lane per (signal, step, class): smoothed, top, score and the candidate flag (is_new = top + 1 or 0);
//   scan_suppress_kernel  a workgroup per signal finds the detections in step order and rewrites is_new with them.
//
// Workspace (tcr_scan_workspace_bytes), regions 256-byte aligned:
//   staging [R][stage_stride] | frame rows [R][n_coef][F + 8] | windows [R G][n_coef][Tp] (2-D graph: planes [R G][T n_coef + 8])
//   | logits, probs [R G][C] | network at R G.
// It does not depend on the signals' length; R and G are derived from the bytes the caller passes.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after stream.hip).
#pragma once
#include <algorithm>

#include "frontend_plan.h"
#include "frontend_args.h"

namespace tcr {

namespace {

constexpr int kScanGroup = 1024;         // steps per front-end row at most (F = G k + T - k frames: T - k recomputed frames per row)
constexpr int kSuppressPer = 32;         // steps per thread and pass of scan_suppress_kernel (256 x 32 = 8192 steps a pass)

struct ScanGeom {
    int G, R, F, T, tp, n_coef, classes, stage_stride;
    bool planes;                // the windows are the 2-D graph's planes
    int64_t win_floats;         // floats of one window (detect_model.h)
    int64_t stage_off, frames_off, win_off, logits_off, probs_off, net_off, ws_floats;     // floats
};

ScanGeom scan_geom(const tcr_frontend_cfg& cfg, const tcr_model_ref& m, const ModelIO& io, int k, int G, int R) {
    ScanGeom g{};
    const int classes = io.classes;
    g.planes = io.planes;
    g.win_floats = model_window_floats(io);
    g.G = G; g.R = R; g.T = cfg.n_frames; g.tp = tcr_padded_len(cfg.n_frames); g.n_coef = cfg.n_coef; g.classes = classes;
    g.F = G * k + g.T - k;
    g.stage_stride = ((g.F - 1) * cfg.hop + cfg.win + 3) / 4 * 4;
    const int64_t B = (int64_t)R * G;
    int64_t o = 0;
    g.stage_off = o; o = align64(o + (int64_t)R * g.stage_stride);
    g.frames_off = o; o = align64(o + (int64_t)R * g.n_coef * tcr_padded_len(g.F));
    g.win_off = o; o = align64(o + B * g.win_floats);
    g.logits_off = o; o = align64(o + B * classes);
    g.probs_off = o; o = align64(o + B * classes);
    g.net_off = o;
    g.ws_floats = o + (int64_t)(model_workspace_bytes(m, (int)B) / sizeof(float));
    return g;
}

// a chunk's slots and frames stay inside the int ranges of the kernels below and of the front-end's launcher, and its R G windows
// inside the batches one network call runs on one kernel path (ModelIO::max_batch: DS-CNN's kDscnnMaxBatch)
bool scan_geom_ok(int k, int T, int G, int64_t R, int max_batch) {
    return R >= 1 && R * G < (1 << 24) && R * G <= max_batch && R * (G * (int64_t)k + T - k) < (1 << 23);
}

}  // namespace

struct ScanStageArgs {
    const float* samples;       // [N][L]
    float* stage;               // [R][stride]
    int64_t L, stride, q0, rows, groups, n_prefix, step_hop;    // step_hop = G k hop (samples between two rows' starts)
    int64_t k_hop;
};

// Staging row r = group q0 + r (signal q / groups, group q % groups): padded samples from frame (g G + 1) k on, i.e. from sample
// (g G + 1) k hop of  zeros(n_prefix) ++ signal ++ zeros.  One thread per staged sample.
__global__ __launch_bounds__(256) void scan_stage_kernel(const ScanStageArgs a) {
    const int64_t total = a.rows * a.stride;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / a.stride, x = e - r * a.stride;
        const int64_t q = a.q0 + r, n = q / a.groups, g = q - n * a.groups;
        const int64_t pos = g * a.step_hop + a.k_hop + x - a.n_prefix;          // sample of the signal
        a.stage[e] = pos >= 0 && pos < a.L ? a.samples[n * a.L + pos] : 0.f;
    }
}

struct ScanGatherArgs {
    const float* frames;        // [R][n_coef][F + 2 kHalo]
    float* windows;             // [R G][n_coef][tp]
    int G, k, T, tp, n_coef, ftp;
};

// One workgroup per window slot b = r G + j: column t of its window is column j k + t of frame row r; the halo is zero.
__global__ __launch_bounds__(256) void scan_gather_kernel(const ScanGatherArgs a) {
    const int b = blockIdx.x;
    const int r = b / a.G, j = b - r * a.G;
    const float* src = a.frames + (size_t)r * a.n_coef * a.ftp + j * a.k;      // window column x <- frame-row column j k + x
    float* dst = a.windows + (size_t)b * a.n_coef * a.tp;
    const int n = a.n_coef * a.tp;
    const int dc = 256 / a.tp, dx = 256 - dc * a.tp;
    int c = threadIdx.x / a.tp, x = threadIdx.x - c * a.tp;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int t = x - kHalo;
        dst[i] = t >= 0 && t < a.T ? src[(size_t)c * a.ftp + x] : 0.f;
        c += dc;
        x += dx;
        if (x >= a.tp) { x -= a.tp; ++c; }
    }
}

// scan_gather_kernel for a 2-D graph: the window of slot b as its [T x n_coef] plane, written in plane order (coalesced): plane
// offset t n_coef + c <- frame-row column j k + t, coefficient c (features_to_plane_kernel's map, net2d_kernels.hip), zero halo.
// A pure copy: bitwise scan_gather_kernel followed by features_to_plane_kernel.
__global__ __launch_bounds__(256) void scan_gather_plane_kernel(const ScanGatherArgs a) {
    const int b = blockIdx.x;
    const int r = b / a.G, j = b - r * a.G;
    const float* src = a.frames + (size_t)r * a.n_coef * a.ftp + j * a.k + kHalo;      // column t <- frame-row column j k + t
    const int n = a.T * a.n_coef, pp = n + 2 * kHalo;
    float* dst = a.windows + (size_t)b * pp;
    for (int i = threadIdx.x; i < pp; i += 256) {
        const int o = i - kHalo;
        float v = 0.f;
        if (o >= 0 && o < n) {
            const int t = o / a.n_coef, c = o - t * a.n_coef;
            v = src[(size_t)c * a.ftp + t];
        }
        dst[i] = v;
    }
}

struct ScanScatterArgs {
    const float* logits_in;     // [R G][C]
    const float* probs_in;
    float* logits;              // [N][steps][C]
    float* probs;
    int64_t q0, groups, steps;
    int G, C, slots;
};

// lane per (slot, class): the slots that are steps of a signal go to the caller's outputs
__global__ __launch_bounds__(256) void scan_scatter_kernel(const ScanScatterArgs a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.slots * a.C) return;
    const int b = (int)(e / a.C), c = (int)(e - (int64_t)b * a.C);
    const int r = b / a.G, j = b - r * a.G;
    const int64_t q = a.q0 + r, n = q / a.groups, g = q - n * a.groups;
    const int64_t i = g * a.G + j;
    if (i >= a.steps) return;
    const int64_t o = (n * a.steps + i) * a.C + c;
    a.logits[o] = a.logits_in[e];
    a.probs[o] = a.probs_in[e];
}

struct ScanSmoothArgs {
    const float* probs;         // [N][steps][C]
    float* smoothed;
    int32_t* top;               // [N][steps]
    float* score;
    int32_t* is_new;            // here: the candidate flag, top + 1 (candidate) or 0
    int64_t windows, steps;
    int C, W, min_count;
    float threshold;
};

// A lane per (signal, step, class), 256 / C steps per workgroup: the streaming detector's smoothing over the last min(i + 1, W)
// probability vectors (smooth_mean, stream.hip: the same expression), the argmax from LDS by the step's first lane, top / score
// (-1 / 0 below min_count) and the candidate flag.  Consecutive lanes read consecutive floats.
__global__ __launch_bounds__(256) void scan_smooth_kernel(const ScanSmoothArgs a) {
    __shared__ float s_sm[256];
    const int C = a.C;
    const int per = 256 / C;
    const int ls = threadIdx.x / C, c = threadIdx.x - ls * C;
    const int64_t w = (int64_t)blockIdx.x * per + ls;                   // window = n steps + i
    const bool live = ls < per && w < a.windows;
    int count = 0;
    if (live) {
        const int64_t i = w % a.steps;
        count = i + 1 < a.W ? (int)(i + 1) : a.W;
        const float* p = a.probs + (w - count + 1) * C + c;             // oldest
        const float v = smooth_mean(count, [&]() {
            const float x = *p;
            p += C;
            return x;
        });
        a.smoothed[w * C + c] = v;
        s_sm[threadIdx.x] = v;
    }
    __syncthreads();
    if (!live || c != 0) return;
    int best = 0;                                                       // (stream_detect_kernel's argmax, written out: as a shared
    float best_v = s_sm[threadIdx.x];                                   // function it reorders that kernel's instructions)
    for (int cc = 1; cc < C; ++cc) {
        const float v = s_sm[threadIdx.x + cc];
        if (v > best_v) { best = cc; best_v = v; }
    }
    const bool warm = count >= a.min_count;
    a.top[w] = warm ? best : -1;
    a.score[w] = warm ? best_v : 0.f;
    a.is_new[w] = warm && best_v > a.threshold ? best + 1 : 0;
}

// One workgroup per signal walks its steps in passes of 256 x kSuppressPer flags, read coalesced into LDS.  A pass without a candidate
// costs its loads and two barriers.  Otherwise wave 0 looks for the next detection: fired = top != prev_label && (prev_label == -1 ||
// i - prev_step > suppression), so after a detection the walk jumps past the suppressed steps, and from there the first candidate whose
// label differs from prev_label fires -- 256 steps per probe (four per lane, the lowest index by a butterfly minimum), one probe per
// detection or per 256 steps.  A detection is marked -1 in LDS; then the candidates' flags are rewritten as 0 / 1.  Non-candidates
// never fire and never change the state.
__global__ __launch_bounds__(256) void scan_suppress_kernel(int32_t* is_new, int64_t steps, int suppression) {
    constexpr int PASS = 256 * kSuppressPer;
    constexpr int NONE = 0x7fffffff;
    __shared__ int s_val[PASS];
    __shared__ int s_any[2];
    const int tid = threadIdx.x;
    int32_t* fl = is_new + (int64_t)blockIdx.x * steps;
    int prev_label = -1;                                // (wave 0's, the same in its lanes)
    int64_t prev_step = 0;
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

namespace {

// the front-end row length for `steps` steps: at most kScanGroup (and max_windows) steps, balanced so the groups of a signal differ
// by at most one step from each other in size
int scan_group(int64_t steps, int cap) {
    const int64_t g0 = std::min<int64_t>(std::min(kScanGroup, cap), steps);
    const int64_t groups = ceil_div64(steps, g0);
    return (int)ceil_div64(steps, groups);
}

// The largest chunk the workspace holds for n_signals x steps: G = the balanced group (smaller when even one row of it does not fit),
// R rows (TCR_ERR_WORKSPACE below one window).  R G also stays within io.max_batch (scan_geom_ok; G <= kScanGroup is far below
// every family's bound), so that every window of a DS-CNN scan runs on the kernel path a stream step of up to kDscnnMaxBatch
// streams runs: the result does not depend on the chunking.
int scan_chunking(const tcr_frontend_cfg& cfg, const tcr_model_ref& m, const ModelIO& io, int k, int64_t steps, int n_signals,
                  size_t ws_bytes, const char* what, ScanGeom& out) {
    int G = scan_group(steps, kScanGroup);
    while (G > 1 && (size_t)scan_geom(cfg, m, io, k, G, 1).ws_floats * sizeof(float) > ws_bytes) G = scan_group(steps, G / 2);
    if ((size_t)scan_geom(cfg, m, io, k, G, 1).ws_floats * sizeof(float) > ws_bytes) {
        set_error("%s: workspace %zu bytes < one window's %zu", what, ws_bytes,
                  (size_t)scan_geom(cfg, m, io, k, 1, 1).ws_floats * sizeof(float));
        return TCR_ERR_WORKSPACE;
    }
    const int64_t total_groups = ceil_div64(steps, G) * n_signals;
    int64_t lo = 1, hi = total_groups;                  // R: the largest that fits (binary search; the size grows with R)
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (scan_geom_ok(k, cfg.n_frames, G, mid, io.max_batch) &&
            (size_t)scan_geom(cfg, m, io, k, G, (int)mid).ws_floats * sizeof(float) <= ws_bytes) lo = mid;
        else hi = mid - 1;
    }
    out = scan_geom(cfg, m, io, k, G, (int)lo);
    return TCR_OK;
}

size_t scan_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_model_ref* m, int k, int max_windows, const char* what) {
    ModelIO io;
    if (stream_check(cfg, m, 1, k, nullptr, what, io) != TCR_OK) return 0;
    if (max_windows < 1) { set_error("%s: max_windows must be >= 1 (got %d)", what, max_windows); return 0; }
    const int G = std::min(kScanGroup, max_windows);
    const int R = max_windows / G;
    if (!scan_geom_ok(k, cfg->n_frames, G, R, io.max_batch)) { set_error("%s: %d windows is too large", what, max_windows); return 0; }
    return (size_t)scan_geom(*cfg, *m, io, k, G, R).ws_floats * sizeof(float);
}

int scan(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* m, int n_signals, int64_t n_samples, int k,
         const tcr_detect_cfg* det, const float* samples, void* workspace, size_t ws_bytes, float* logits, float* probs, float* smoothed,
         int32_t* top, float* score, int32_t* is_new, void* stream, const char* what) {
    TCR_REQUIRE(plan_dev && m && m->params && m->aux && det && samples && workspace && logits && probs && smoothed && top && score && is_new,
                "%s: null argument", what);
    TCR_REQUIRE(n_signals > 0, "%s: the number of signals must be positive (got %d)", what, n_signals);
    ModelIO io;
    TCR_TRY(stream_check(cfg, m, n_signals, k, det, what, io, false));
    const int64_t khop = (int64_t)k * cfg->hop;
    TCR_REQUIRE(n_samples > 0 && n_samples % khop == 0, "%s: the signal length %lld is not a positive multiple of k * hop = %lld", what,
                (long long)n_samples, (long long)khop);
    const int64_t steps = n_samples / khop;
    TCR_REQUIRE((int64_t)n_signals * steps * io.classes < ((int64_t)1 << 31), "%s: %d signals x %lld steps is too large", what, n_signals,
                (long long)steps);
    ScanGeom g;
    TCR_TRY(scan_chunking(*cfg, *m, io, k, steps, n_signals, ws_bytes, what, g));
    const int G = g.G;
    const int64_t groups = ceil_div64(steps, G), total_groups = groups * n_signals;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* ws = static_cast<float*>(workspace);
    const int ftp = tcr_padded_len(g.F);
    for (int64_t q0 = 0; q0 < total_groups; q0 += g.R) {
        const int rows = (int)std::min<int64_t>(g.R, total_groups - q0);
        const int slots = rows * G;
        ScanStageArgs sa;
        sa.samples = samples; sa.stage = ws + g.stage_off; sa.L = n_samples; sa.stride = g.stage_stride; sa.q0 = q0; sa.rows = rows;
        sa.groups = groups; sa.n_prefix = cfg->n_samples; sa.step_hop = (int64_t)G * khop; sa.k_hop = khop;
        const int64_t staged = (int64_t)rows * g.stage_stride;
        hipLaunchKernelGGL(scan_stage_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(staged, 256), 8 * (int64_t)device_cus())), dim3(256), 0,
                           s, sa);
        TCR_TRY(check_launch("scan_stage_kernel"));
        TCR_TRY(stream_frontend(*cfg, plan_dev, ws + g.stage_off, g.stage_stride, rows, g.F, ws + g.frames_off, s, ftp));
        ScanGatherArgs ga;
        ga.frames = ws + g.frames_off; ga.windows = ws + g.win_off; ga.G = G; ga.k = k; ga.T = g.T; ga.tp = g.tp; ga.n_coef = g.n_coef;
        ga.ftp = ftp;
        if (g.planes) {
            hipLaunchKernelGGL(scan_gather_plane_kernel, dim3(slots), dim3(256), 0, s, ga);
            TCR_TRY(check_launch("scan_gather_plane_kernel"));
        } else {
            hipLaunchKernelGGL(scan_gather_kernel, dim3(slots), dim3(256), 0, s, ga);
            TCR_TRY(check_launch("scan_gather_kernel"));
        }
        TCR_TRY(model_forward(*m, ws + g.win_off, slots, ws + g.net_off, ws_bytes - (size_t)g.net_off * sizeof(float), ws + g.logits_off,
                              ws + g.probs_off, stream));
        ScanScatterArgs xa;
        xa.logits_in = ws + g.logits_off; xa.probs_in = ws + g.probs_off; xa.logits = logits; xa.probs = probs; xa.q0 = q0;
        xa.groups = groups; xa.steps = steps; xa.G = G; xa.C = g.classes; xa.slots = slots;
        hipLaunchKernelGGL(scan_scatter_kernel, dim3(ceil_div(slots * g.classes, 256)), dim3(256), 0, s, xa);
        TCR_TRY(check_launch("scan_scatter_kernel"));
    }
    ScanSmoothArgs ma;
    ma.probs = probs; ma.smoothed = smoothed; ma.top = top; ma.score = score; ma.is_new = is_new; ma.windows = (int64_t)n_signals * steps;
    ma.steps = steps; ma.C = g.classes; ma.W = det->average_steps; ma.min_count = det->min_count; ma.threshold = det->threshold;
    hipLaunchKernelGGL(scan_smooth_kernel, dim3((unsigned)ceil_div64(ma.windows, 256 / g.classes)), dim3(256), 0, s, ma);
    TCR_TRY(check_launch("scan_smooth_kernel"));
    hipLaunchKernelGGL(scan_suppress_kernel, dim3(n_signals), dim3(256), 0, s, is_new, steps, det->suppression_steps);
    return check_launch("scan_suppress_kernel");
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" size_t tcr_scan_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_net* net, int k, int max_windows) {
    const tcr_model_ref m = tcresnet_ref(net, nullptr, nullptr);
    return scan_workspace_bytes(cfg, &m, k, max_windows, "tcr_scan_workspace_bytes");
}

extern "C" size_t tcr_scan_workspace_bytes_m(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int k, int max_windows) {
    return scan_workspace_bytes(cfg, model, k, max_windows, "tcr_scan_workspace_bytes_m");
}

extern "C" int tcr_scan(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params, const float* frozen_ss,
                        int n_signals, int64_t n_samples, int k, const tcr_detect_cfg* det, const float* samples, void* workspace,
                        size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                        void* stream) {
    const tcr_model_ref m = tcresnet_ref(net, params, frozen_ss);
    return scan(cfg, plan_dev, &m, n_signals, n_samples, k, det, samples, workspace, ws_bytes, logits, probs, smoothed, top, score, is_new,
                stream, "tcr_scan");
}

extern "C" int tcr_scan_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_signals, int64_t n_samples,
                          int k, const tcr_detect_cfg* det, const float* samples, void* workspace, size_t ws_bytes, float* logits,
                          float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    return scan(cfg, plan_dev, model, n_signals, n_samples, k, det, samples, workspace, ws_bytes, logits, probs, smoothed, top, score, is_new,
                stream, "tcr_scan_m");
}
