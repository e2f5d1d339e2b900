// Streaming keyword spotting over many concurrent audio streams (tcr_stream_*): per step, every stream hears k * hop new samples,
// only the k new MFCC / log-mel frames are computed, the network runs on the window kept on the device, and the posteriors are
// smoothed into detections there.
//
// Each stream conceptually carries audio = zeros(n_samples) ++ everything pushed since its last reset; after a step its window is
// bitwise the ordinary front-end's features of audio[-n_samples:], because
//   * a window column is a pure function of its frame's samples (frontend_pk3.hip: the same operations on every frame), so the
//     columns that survive a step move left by k unchanged, and
//   * the k new frames are computed by frontend_pk3_kernel's streaming instance from a staging row that holds exactly the samples
//     they cover: tail ++ new, where tail = the last  win - hop + ((n_samples - win) mod hop)  samples heard (the new clip ends
//     (n_samples - win) mod hop samples behind its last frame, so the staging row's first sample is the first new frame's first).
//     With hop > win that count can be negative: the first  hop - win - ((n_samples - win) mod hop)  samples of a step lie in the gap
//     between two frames and belong to none.  The state then keeps no tail (tail_len = 0) and the staging row starts that many
//     samples (skip) into the step's new ones.  tail_len and skip are never both positive.
// Nothing is accumulated: every column comes from raw samples, so the window does not drift however long a stream runs.
//
// Kernels of a step: stream_stage_kernel (reset, staging row, tail, window shift; one workgroup per stream, so the in-place shift has
// no cross-workgroup hazard), frontend_pk3_kernel<.., STREAM = true>, the network (detect_model.h: tcr_net_forward_frozen,
// tcr_dscnn_forward_infer on the planar windows, or tcr_g2d_forward_infer on planes that features_to_plane_kernel lays out from them
// in the workspace; the state keeps the planar window whatever the family, the front-end writes its new columns there), then
// stream_detect_kernel (a lane per stream and class: the smoothing / detection rule of the header, a ring of the last W probability
// vectors).
//
// State (caller-owned device memory, tcr_stream_state_bytes), regions 256-byte aligned:
//   window [S][n_coef][T + 2 TCR_HALO] | zero window [n_coef][Tp] (the features of a silent clip: what a reset window is)
//   | tail [S][tail_len] | ring [W][S][classes] | detector integers [5][S] (head, count, prev_label, prev_step, n)
// Workspace (tcr_stream_workspace_bytes): staging rows [S][stage_stride] (>= n_samples floats) | 2-D graph: the planes
//   [S][T n_coef + 2 TCR_HALO] | the network's workspace at batch S.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, next to the streaming front-end's launcher).
#pragma once
#include <algorithm>
#include <cstdio>

#include "frontend_plan.h"
#include "frontend_args.h"
#include "detect_model.h"

namespace tcr {

namespace {

constexpr int kMaxTail = 1024;          // 0 <= tail_len <= win - 1 < nfft <= 1024 (hop > win: max(win - hop + remainder, 0))
constexpr int kShiftRegs = 8;           // window elements per thread and pass of the shift

struct StreamGeom {
    int S, k, T, tp, n_coef, classes, W;
    int tail_len, skip, stage_stride;   // samples kept per stream; samples of a step in front of its first new frame (hop > win)
    int64_t win_off, zw_off, tail_off, ring_off, ist_off, state_floats;         // state offsets in floats
    int64_t stage_floats, plane_off, net_ws_off, ws_floats;                     // workspace
};

int64_t align64(int64_t v) { return (v + 63) / 64 * 64; }     // floats -> 256 bytes

// Where a step's new samples start, counted from the first new frame's first sample: win - hop + ((n_samples - win) mod hop).
// Positive: that many samples heard before the step are part of the new frames (the tail).  Negative (hop > win only): the step's
// first -that many samples belong to no frame.
int stream_tail_samples(const tcr_frontend_cfg& cfg) { return cfg.win - cfg.hop + (cfg.n_samples - cfg.win) % cfg.hop; }

StreamGeom stream_geom(const tcr_frontend_cfg& cfg, const tcr_model_ref& m, const ModelIO& io, int S, int k, int W) {
    StreamGeom g{};
    const int classes = io.classes;
    g.S = S; g.k = k; g.T = cfg.n_frames; g.tp = tcr_padded_len(cfg.n_frames); g.n_coef = cfg.n_coef; g.classes = classes; g.W = W;
    const int behind = stream_tail_samples(cfg);
    g.tail_len = std::max(behind, 0);
    g.skip = std::max(-behind, 0);
    g.stage_stride = (g.tail_len + k * cfg.hop - g.skip + 3) / 4 * 4;          // >= (k - 1) hop + win: the k new frames
    int64_t o = 0;
    g.win_off = o; o = align64(o + (int64_t)S * g.n_coef * g.tp);
    g.zw_off = o; o = align64(o + (int64_t)g.n_coef * g.tp);
    g.tail_off = o; o = align64(o + (int64_t)S * g.tail_len);
    g.ring_off = o; o = align64(o + (int64_t)W * classes * S);
    g.ist_off = o; o = align64(o + 5 * (int64_t)S);
    g.state_floats = o;
    g.stage_floats = align64(std::max((int64_t)S * g.stage_stride, (int64_t)cfg.n_samples));
    g.plane_off = g.stage_floats;
    g.net_ws_off = g.plane_off + (io.planes ? align64((int64_t)S * model_window_floats(io)) : 0);
    g.ws_floats = g.net_ws_off + (int64_t)(model_workspace_bytes(m, S) / sizeof(float));
    return g;
}

// Everything the create / step calls refuse, with the reason; io: the network's shape.  S is a batch of the network (the streams of
// tcr_stream_*), or not (the signals of tcr_scan: streams_are_batch = false).
int stream_check(const tcr_frontend_cfg* cfg, const tcr_model_ref* m, int S, int k, const tcr_detect_cfg* det, const char* what, ModelIO& io,
                 bool streams_are_batch = true) {
    TCR_REQUIRE(cfg && m && m->handle, "%s: null front-end configuration or network", what);
    TCR_TRY(model_io(*m, what, io));
    TCR_REQUIRE(cfg->nfft == 512 || cfg->nfft == 1024, "%s: unresolved or unsupported front-end configuration (nfft=%d)", what, cfg->nfft);
    TCR_REQUIRE(cfg->method != 2, "%s: the float64 deploy front-end (method 2, mfcc_deploy) has no streaming instance", what);
    TCR_REQUIRE(cfg->n_coef == io.n_coef && cfg->n_frames == io.t, "%s: the front-end yields %d x %d features, the network expects %d x %d",
                what, cfg->n_coef, cfg->n_frames, io.n_coef, io.t);
    TCR_REQUIRE(S > 0, "%s: the number of streams must be positive (got %d)", what, S);
    TCR_REQUIRE(!streams_are_batch || S <= io.max_batch, "%s: %d streams exceed the %d windows one call of this network runs", what, S,
                io.max_batch);
    TCR_REQUIRE(io.classes <= 256, "%s: the detector takes at most 256 classes (got %d)", what, io.classes);
    TCR_REQUIRE(k >= 1 && k <= cfg->n_frames, "%s: frames per step k = %d outside 1..T = %d", what, k, cfg->n_frames);
    TCR_REQUIRE((int64_t)S * k < (1 << 23) && (int64_t)S * cfg->n_frames < ((int64_t)1 << 31), "%s: %d streams x %d frames is too large", what, S, k);
    // (n_items = 0: the window / hop part of the launcher's test alone, so that the two causes are told apart)
    TCR_REQUIRE((cfg->hop & 1) == 0 && frontend_pk3_supports(cfg->nfft / 2, cfg->win, 0),
                "%s: the streaming front-end (frontend_pk3_kernel) does not cover window %d / hop %d / %d mel bands at nfft %d; another "
                "kernel would not give the offline features bitwise", what, cfg->win, cfg->hop, cfg->n_mel, cfg->nfft);
    // (an odd clip: the offline front-end runs its general kernel, frontend.hip's `aligned`; the streaming instance would decline late)
    TCR_REQUIRE((cfg->n_samples & 1) == 0, "%s: the streaming front-end (frontend_pk3_kernel) does not cover a clip of %d samples (an odd "
                "clip length: the offline front-end runs another kernel on it, which would not give the streamed features bitwise)", what,
                cfg->n_samples);
    {
        const int n_items = frontend_mel_item_count(*cfg), n_fast = mel_items_fast(cfg->nfft / 2);
        char why[160];
        if (n_items < 0)
            std::snprintf(why, sizeof(why), "a mel-edge segment of more than %d bins (three work items; the kernel's log phase reads no more)",
                          3 * mel_item_bins(cfg->nfft / 2));
        else
            std::snprintf(why, sizeof(why), "%d work items, its unrolled trips take %d", n_items, n_fast);
        TCR_REQUIRE(frontend_pk3_supports(cfg->nfft / 2, cfg->win, n_items),
                    "%s: the streaming front-end (frontend_pk3_kernel) does not cover the mel filterbank %g - %g Hz at sample rate %d / "
                    "nfft %d (%s); another kernel would not give the offline features bitwise", what, cfg->lower_hz, cfg->upper_hz,
                    cfg->sample_rate, cfg->nfft, why);
    }
    TCR_REQUIRE(stream_tail_samples(*cfg) <= kMaxTail, "%s: window %d / hop %d leave a tail of more than %d samples", what, cfg->win,
                cfg->hop, kMaxTail);
    if (det) {
        TCR_REQUIRE(det->average_steps >= 1, "%s: average_steps (the ring of probability vectors) must be >= 1 (got %d)", what, det->average_steps);
        TCR_REQUIRE(det->min_count >= 1 && det->min_count <= det->average_steps, "%s: min_count %d outside 1..average_steps = %d", what,
                    det->min_count, det->average_steps);
        TCR_REQUIRE(det->suppression_steps >= 0, "%s: suppression_steps must be >= 0 (got %d)", what, det->suppression_steps);
    }
    return TCR_OK;
}

}  // namespace

struct StageArgs {
    const float* samples;       // [S][k hop]
    const uint8_t* reset;       // [S] or null
    float* window;              // [S][n_coef][tp]
    const float* zw;            // [n_coef][tp]
    float* tail;                // [S][tail_len]
    float* stage;               // [S][stage_stride]
    int khop, tail_len, skip, stage_stride, n_coef, tp, T, k;
};

// The staging arguments of a step over the state at st (tcr_stream_step, tcr_stream_step_selected_m).
static StageArgs stage_args(const StreamGeom& g, const tcr_frontend_cfg& cfg, const float* samples, const uint8_t* reset, float* st, float* stage) {
    StageArgs sa;
    sa.samples = samples; sa.reset = reset; sa.window = st + g.win_off; sa.zw = st + g.zw_off; sa.tail = st + g.tail_off; sa.stage = stage;
    sa.khop = g.k * cfg.hop; sa.tail_len = g.tail_len; sa.skip = g.skip; sa.stage_stride = g.stage_stride; sa.n_coef = g.n_coef; sa.tp = g.tp;
    sa.T = g.T; sa.k = g.k;
    return sa;
}

// One workgroup per stream: reset, staging row tail ++ new samples (from sample `skip` of the new ones on: tail_len = 0 then), the new
// tail, the window's columns k..T-1 moved to 0..T-k-1 (the front-end then writes columns T-k..T-1).  The old tail is read into LDS before the new one is written; the shift moves the window
// in passes of 256 x kShiftRegs elements in row order, each read into registers before a barrier and written behind it -- a later
// pass only reads columns (>= t + k of a row) that no earlier pass writes.
__global__ __launch_bounds__(256) void stream_stage_kernel(const StageArgs a) {
    __shared__ float s_tail[kMaxTail];
    const int s = blockIdx.x;
    const int tid = threadIdx.x;
    const bool rst = a.reset && a.reset[s];
    float* tail = a.tail + (size_t)s * a.tail_len;
    const float* src = a.samples + (size_t)s * a.khop;
    for (int i = tid; i < a.tail_len; i += 256) s_tail[i] = rst ? 0.f : tail[i];
    __syncthreads();
    float* stage = a.stage + (size_t)s * a.stage_stride;
    const float* fresh = src + a.skip;          // the new samples from the first new frame's first sample on
    for (int i = tid; i < a.tail_len + a.khop - a.skip; i += 256) stage[i] = i < a.tail_len ? s_tail[i] : fresh[i - a.tail_len];
    for (int i = tid; i < a.tail_len; i += 256) {
        const int j = i + a.khop;
        tail[i] = j < a.tail_len ? s_tail[j] : src[j - a.tail_len];
    }
    const int keep = a.T - a.k;                 // surviving columns per row
    const int n = a.n_coef * keep;
    const float inv_keep = keep > 0 ? 1.0f / (float)keep : 0.f;
    float* win = a.window + (size_t)s * a.n_coef * a.tp + kHalo;
    const float* zw = a.zw + kHalo;
    for (int base = 0; base < n; base += 256 * kShiftRegs) {
        float v[kShiftRegs];
#pragma unroll
        for (int m = 0; m < kShiftRegs; ++m) {
            const int i = base + m * 256 + tid;
            if (i < n) {
                const int c = fast_div(i, keep, inv_keep), t = i - c * keep;
                const int at = c * a.tp + t + a.k;
                v[m] = rst ? zw[at] : win[at];
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kShiftRegs; ++m) {
            const int i = base + m * 256 + tid;
            if (i < n) {
                const int c = fast_div(i, keep, inv_keep), t = i - c * keep;
                win[c * a.tp + t] = v[m];
            }
        }
    }
}

// Every stream = the silent clip: window = the zero window, tail zero, detector state fresh.
__global__ __launch_bounds__(256) void stream_init_kernel(float* window, const float* zw, int win_elems, int S, float* tail, int tail_len,
                                                          int* ist) {
    const int64_t total = (int64_t)S * win_elems;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) window[i] = zw[i % win_elems];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (int64_t)S * tail_len; i += (int64_t)gridDim.x * 256) tail[i] = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S; i += (int64_t)gridDim.x * 256) {
        ist[i] = 0;                 // head
        ist[S + i] = 0;             // count
        ist[2 * S + i] = -1;        // prev_label
        ist[3 * S + i] = 0;         // prev_step
        ist[4 * S + i] = 0;         // n
    }
}

// The detector's smoothing (tcr_stream_step): `count` values of one class, oldest to newest (next() yields them in that order), summed
// in float32 -- the loads requested eight at a time, the adds in order -- times (1.0f / count).  stream_detect_kernel and
// scan_smooth_kernel (scan.hip) both call it, so an offline scan smooths with the streaming detector's expression.
template <class Next>
__device__ __forceinline__ float smooth_mean(int count, Next next) {
    float acc = 0.f;
    int i = 0;
    for (; i + 8 <= count; i += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = next();
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += v[j];
    }
    for (; i < count; ++i) acc += next();
    return acc * (1.0f / (float)count);
}

struct DetectArgs {
    const float* probs;         // [S][C]
    const uint8_t* reset;
    float* ring;                // [W][S][C]
    int* ist;                   // [5][S]
    float* smoothed;            // [S][C]
    int* top;
    float* score;
    int* is_new;
    int S, C, W, min_count, suppression;
    float threshold;
};

// A lane per (stream, class): a workgroup holds 256 / C streams.  Each lane stores its class's probability into the ring slot and
// sums the ring oldest to newest in float32 (the loads requested eight at a time, the adds in ring order); the stream's first lane
// takes the argmax (lowest index on ties) from LDS and runs the detection rule of tcr_stream_step's documentation.  Ring
// [W][S][C]: a wave's accesses are contiguous.
__global__ __launch_bounds__(256) void stream_detect_kernel(const DetectArgs a) {
    __shared__ float s_sm[256];
    const int S = a.S, C = a.C, W = a.W;
    const int per = 256 / C;                    // streams per workgroup
    const int ls = threadIdx.x / C, c = threadIdx.x - ls * C;
    const int s = blockIdx.x * per + ls;
    const bool live = ls < per && s < S;
    int head = 0, count = 0, prev_label = -1, prev_step = 0, n = 0;
    if (live) {
        head = a.ist[s]; count = a.ist[S + s]; prev_label = a.ist[2 * S + s]; prev_step = a.ist[3 * S + s]; n = a.ist[4 * S + s];
        if (a.reset && a.reset[s]) { head = 0; count = 0; prev_label = -1; prev_step = 0; n = 0; }
        const size_t sc = (size_t)s * C + c, ring_row = (size_t)S * C;
        a.ring[head * ring_row + sc] = a.probs[sc];
        head = head + 1 == W ? 0 : head + 1;
        count = min(count + 1, W);
        int slot = head - count < 0 ? head - count + W : head - count;        // oldest
        const float v = smooth_mean(count, [&]() {
            const float x = a.ring[slot * ring_row + sc];
            slot = slot + 1 == W ? 0 : slot + 1;
            return x;
        });
        a.smoothed[sc] = v;
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
    int top = -1, fired = 0;
    float score = 0.f;
    if (count >= a.min_count) {
        top = best;
        score = best_v;
        fired = score > a.threshold && top != prev_label && (prev_label == -1 || n - prev_step > a.suppression);
        if (fired) { prev_label = top; prev_step = n; }
    }
    n += 1;
    a.top[s] = top;
    a.score[s] = score;
    a.is_new[s] = fired;
    a.ist[s] = head; a.ist[S + s] = count; a.ist[2 * S + s] = prev_label; a.ist[3 * S + s] = prev_step; a.ist[4 * S + s] = n;
}

namespace {

// the streaming front-end over `rows` staging rows of `stride` floats, k frames each, into columns tp - 8 - k .. tp - 9 of rows of tp
// columns (tp = 0: the window's T + 2 TCR_HALO, i.e. columns T - k .. T - 1; tcr_scan passes k + 2 TCR_HALO: columns 0 .. k - 1)
int stream_frontend(const tcr_frontend_cfg& cfg, const void* plan_dev, const float* stage, int stride, int rows, int k, float* out,
                    hipStream_t s, int tp = 0) {
    FrontendArgs a;
    frontend_plan_args(&cfg, plan_dev, a);
    a.wav = stage;
    a.out = out;
    a.n_samples = stride;
    a.win = cfg.win;
    a.hop = cfg.hop;
    a.n_frames = k;
    a.n_coef = cfg.n_coef;
    a.tp = tp > 0 ? tp : tcr_padded_len(cfg.n_frames);
    a.total_frames = rows * k;
    a.magnitude = cfg.method != 0;
    a.no_dct = cfg.method == 1;
    a.log_floor = 0;
    // one round of frames per persistent-workgroup chunk while the chunks fit one generation of the CUs' slots (a step's few frames:
    // as many workgroups as there are rounds); otherwise the launcher's cost model.  The features do not depend on it.
    a.rounds = ceil_div(a.total_frames, 4096 / (cfg.nfft / 2)) <= 3 * device_cus() ? 1 : 0;
    a.stagger = 0;
    a.stagger_div = 1;
    a.aligned = (stride & 1) == 0 && (cfg.hop & 1) == 0 && (reinterpret_cast<uintptr_t>(stage) & 7) == 0;
    const int rc = launch_frontend_pk3_stream(cfg.nfft / 2, a, frontend_mel_item_count(cfg), s);
    TCR_REQUIRE(rc != 1, "tcr_stream: frontend_pk3_kernel declined the configuration");
    return rc;
}

size_t stream_state_bytes(const tcr_frontend_cfg* cfg, const tcr_model_ref* m, int n_streams, int k, const tcr_detect_cfg* det,
                          const char* what) {
    if (!det) { set_error("%s: null detector configuration", what); return 0; }
    ModelIO io;
    if (stream_check(cfg, m, n_streams, k, det, what, io) != TCR_OK) return 0;
    return (size_t)stream_geom(*cfg, *m, io, n_streams, k, det->average_steps).state_floats * sizeof(float);
}

size_t stream_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_model_ref* m, int n_streams, int k, const char* what) {
    ModelIO io;
    if (stream_check(cfg, m, n_streams, k, nullptr, what, io) != TCR_OK) return 0;
    return (size_t)stream_geom(*cfg, *m, io, n_streams, k, 1).ws_floats * sizeof(float);
}

int stream_init(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* m, int n_streams, int k, const tcr_detect_cfg* det,
                void* state, void* workspace, size_t ws_bytes, void* stream, const char* what) {
    TCR_REQUIRE(plan_dev && det && state && workspace, "%s: null argument", what);
    ModelIO io;
    TCR_TRY(stream_check(cfg, m, n_streams, k, det, what, io));
    const StreamGeom g = stream_geom(*cfg, *m, io, n_streams, k, det->average_steps);
    if ((size_t)g.ws_floats * sizeof(float) > ws_bytes) {
        set_error("%s: workspace %zu bytes < required %zu", what, ws_bytes, (size_t)g.ws_floats * sizeof(float));
        return TCR_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* st = static_cast<float*>(state);
    float* ws = static_cast<float*>(workspace);
    // the zero window: the streaming front-end over one silent clip (all T frames, columns 0..T-1) -- the offline kernel's arithmetic
    if (hipMemsetAsync(ws, 0, (size_t)cfg->n_samples * sizeof(float), s) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", what);
        return TCR_ERR_HIP;
    }
    TCR_TRY(stream_frontend(*cfg, plan_dev, ws, cfg->n_samples, 1, cfg->n_frames, st + g.zw_off, s));
    if (hipMemsetAsync(st + g.ring_off, 0, (size_t)g.W * g.classes * g.S * sizeof(float), s) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", what);
        return TCR_ERR_HIP;
    }
    const int64_t work = (int64_t)g.S * g.n_coef * g.tp;
    const int grid = (int)std::min<int64_t>(ceil_div64(work, 256), 4 * (int64_t)device_cus());
    hipLaunchKernelGGL(stream_init_kernel, dim3(grid), dim3(256), 0, s, st + g.win_off, st + g.zw_off, g.n_coef * g.tp, g.S,
                       st + g.tail_off, g.tail_len, reinterpret_cast<int*>(st + g.ist_off));
    return check_launch("stream_init_kernel");
}

int stream_step(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* m, int n_streams, int k, const tcr_detect_cfg* det,
                const float* samples, const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, float* logits, float* probs,
                float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream, const char* what) {
    TCR_REQUIRE(plan_dev && m && m->params && m->aux && det && samples && state && workspace && logits && probs && smoothed && top && score &&
                is_new, "%s: null argument", what);
    ModelIO io;
    TCR_TRY(stream_check(cfg, m, n_streams, k, det, what, io));
    const StreamGeom g = stream_geom(*cfg, *m, io, n_streams, k, det->average_steps);
    if ((size_t)g.ws_floats * sizeof(float) > ws_bytes) {
        set_error("%s: workspace %zu bytes < required %zu", what, ws_bytes, (size_t)g.ws_floats * sizeof(float));
        return TCR_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* st = static_cast<float*>(state);
    float* ws = static_cast<float*>(workspace);
    const StageArgs sa = stage_args(g, *cfg, samples, reset, st, ws);
    hipLaunchKernelGGL(stream_stage_kernel, dim3(g.S), dim3(256), 0, s, sa);
    TCR_TRY(check_launch("stream_stage_kernel"));
    TCR_TRY(stream_frontend(*cfg, plan_dev, ws, g.stage_stride, g.S, k, st + g.win_off, s));
    const float* x = st + g.win_off;
    if (io.planes) {            // the 2-D graph's planes, relaid out from the windows (a pure copy)
        TCR_TRY(tcr_g2d_input_from_features(x, g.S, g.T, g.n_coef, ws + g.plane_off, stream));
        x = ws + g.plane_off;
    }
    TCR_TRY(model_forward(*m, x, g.S, ws + g.net_ws_off, ws_bytes - (size_t)g.net_ws_off * sizeof(float), logits, probs, stream));
    DetectArgs da;
    da.probs = probs; da.reset = reset; da.ring = st + g.ring_off; da.ist = reinterpret_cast<int*>(st + g.ist_off);
    da.smoothed = smoothed; da.top = top; da.score = score; da.is_new = is_new;
    da.S = g.S; da.C = g.classes; da.W = g.W; da.min_count = det->min_count; da.suppression = det->suppression_steps; da.threshold = det->threshold;
    hipLaunchKernelGGL(stream_detect_kernel, dim3(ceil_div(g.S, 256 / g.classes)), dim3(256), 0, s, da);
    return check_launch("stream_detect_kernel");
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" size_t tcr_stream_state_bytes(const tcr_frontend_cfg* cfg, const tcr_net* net, int n_streams, int k, const tcr_detect_cfg* det) {
    const tcr_model_ref m = tcresnet_ref(net, nullptr, nullptr);
    return stream_state_bytes(cfg, &m, n_streams, k, det, "tcr_stream_state_bytes");
}

extern "C" size_t tcr_stream_state_bytes_m(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int n_streams, int k,
                                           const tcr_detect_cfg* det) {
    return stream_state_bytes(cfg, model, n_streams, k, det, "tcr_stream_state_bytes_m");
}

extern "C" size_t tcr_stream_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_net* net, int n_streams, int k) {
    const tcr_model_ref m = tcresnet_ref(net, nullptr, nullptr);
    return stream_workspace_bytes(cfg, &m, n_streams, k, "tcr_stream_workspace_bytes");
}

extern "C" size_t tcr_stream_workspace_bytes_m(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int n_streams, int k) {
    return stream_workspace_bytes(cfg, model, n_streams, k, "tcr_stream_workspace_bytes_m");
}

extern "C" int tcr_stream_init(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, int n_streams, int k,
                               const tcr_detect_cfg* det, void* state, void* workspace, size_t ws_bytes, void* stream) {
    const tcr_model_ref m = tcresnet_ref(net, nullptr, nullptr);
    return stream_init(cfg, plan_dev, &m, n_streams, k, det, state, workspace, ws_bytes, stream, "tcr_stream_init");
}

extern "C" int tcr_stream_init_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams, int k,
                                 const tcr_detect_cfg* det, void* state, void* workspace, size_t ws_bytes, void* stream) {
    return stream_init(cfg, plan_dev, model, n_streams, k, det, state, workspace, ws_bytes, stream, "tcr_stream_init_m");
}

extern "C" int tcr_stream_step(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                               const float* frozen_ss, int n_streams, int k, const tcr_detect_cfg* det, const float* samples,
                               const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, float* logits, float* probs,
                               float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    const tcr_model_ref m = tcresnet_ref(net, params, frozen_ss);
    return stream_step(cfg, plan_dev, &m, n_streams, k, det, samples, reset, state, workspace, ws_bytes, logits, probs, smoothed, top, score,
                       is_new, stream, "tcr_stream_step");
}

extern "C" int tcr_stream_step_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams, int k,
                                 const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state, void* workspace,
                                 size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                                 void* stream) {
    return stream_step(cfg, plan_dev, model, n_streams, k, det, samples, reset, state, workspace, ws_bytes, logits, probs, smoothed, top, score,
                       is_new, stream, "tcr_stream_step_m");
}
