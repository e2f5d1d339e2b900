// Streaming cascades: the causal cascade (scan_select.hip, pad_before = 0) carried from push to push.  A cheap detector steps every
// stream; tcr_stream_select picks the streams a second detector should look at; tcr_stream_step_selected_m is a step of that second
// detector which advances all S windows but runs its network on the selected streams only.
//
// tcr_stream_select: stream s is flagged when a masked class has values[s][c] >= enter, and selected when it was flagged at this step
// or at one of the pad_after steps before it since its last reset -- tcr_scan_select's rule at pad_before = 0, a stream's steps being
// a signal's.  The carried state is one int32 per stream, `since`: the steps since its last flag, saturating, INT32_MAX = never.
//   stream_flag_kernel     a lane per (stream, class), as select_flag_kernel reads values; the stream's first lane applies the reset,
//                          advances `since` and writes the selection byte (and `mask`);
//   select_count_kernel, select_scan_kernel (which writes n_selected), select_compact_kernel over the S bytes: the selected streams
//                          in increasing order (scan_select.hip's prefix sums; no atomics, no workgroup waits for another).
// No floating-point arithmetic beyond the compare.
//
// tcr_stream_step_selected_m, on an ordinary tcr_stream_init_m state:
//   stream_stage_kernel, frontend_pk3_kernel    for all S streams, exactly as tcr_stream_step_m launches them: every window and tail;
//   stream_gather_kernel   <PLANES>: slot b of the workspace <- the window of stream selected[b] (16 bytes a lane where n_coef x tp
//                          and the pointers allow it; PLANES: straight into the 2-D graph's plane order, features_to_plane_kernel's map);
//   the network at batch n_selected on the slots, into compact rows of the workspace;
//   stream_merge_kernel    a lane per (stream, class): the stream's slot by a binary search of `selected` (its first lane; the others
//                          read it from LDS), then its logits / probs row from the compact rows or from the caller's fill rows;
//   stream_detect_kernel   unchanged, over the merged probs of all S streams.
// All S selected: no gather and no merge -- the network reads the state's windows and writes the caller's rows, the launches of
// tcr_stream_step_m.  None selected: no gather and no network, the merge copies the fill rows.
// Workspace: staging rows | slots [S][window floats] | compact logits, probs [S][C] each | the network's workspace at batch S.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end).
#pragma once
#include <climits>

namespace tcr {

struct StreamFlagArgs {
    const float* values;        // [S][C]
    const uint8_t* class_mask;  // [C]
    const uint8_t* reset;       // [S] or null
    int32_t* since;             // [S]
    uint8_t* bits;              // [S]: the selection
    uint8_t* mask;              // [S] or null
    int S, C, pad_after;
    float enter;
};

// A lane per (stream, class), 256 / C streams per workgroup; a float32 compare, so a NaN never flags.
__global__ __launch_bounds__(256) void stream_flag_kernel(const StreamFlagArgs a) {
    __shared__ int s_f[256];
    const int C = a.C, per = 256 / C;
    const int ls = threadIdx.x / C, c = threadIdx.x - ls * C;
    const int s = blockIdx.x * per + ls;
    const bool live = ls < per && s < a.S;
    int f = 0;
    if (live) f = a.class_mask[c] != 0 && a.values[(size_t)s * C + c] >= a.enter;
    s_f[threadIdx.x] = f;
    __syncthreads();
    if (!live || c != 0) return;
    for (int cc = 1; cc < C; ++cc) f |= s_f[threadIdx.x + cc];
    int since = a.since[s];
    if (a.reset && a.reset[s]) since = INT32_MAX;
    since = f ? 0 : (since == INT32_MAX ? INT32_MAX : since + 1);
    a.since[s] = since;
    const uint8_t sel = since != INT32_MAX && since <= a.pad_after ? 1 : 0;
    a.bits[s] = sel;
    if (a.mask) a.mask[s] = sel;
}

__global__ __launch_bounds__(256) void stream_since_init_kernel(int32_t* since, int S) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < S) since[s] = INT32_MAX;
}

struct StreamGatherArgs {
    const float* window;        // [S][n_coef][tp]
    const int64_t* selected;    // [n]
    float* slots;               // [n][n_coef][tp] (planes: [n][T n_coef + 2 kHalo])
    int S, n_coef, tp, T;
    int vec;                    // 16 bytes a lane: n_coef x tp a multiple of four floats, both pointers 16-byte aligned
};

// One workgroup per slot b: the window of stream selected[b], a plain copy; PLANES: plane offset t n_coef + c <- window column t,
// coefficient c, the halo zero (features_to_plane_kernel).  A stream index outside 0 .. S - 1 (a broken precondition) copies nothing.
template <bool PLANES>
__global__ __launch_bounds__(256) void stream_gather_kernel(const StreamGatherArgs a) {
    const int b = blockIdx.x;
    const int64_t s = a.selected[b];
    if (s < 0 || s >= a.S) return;
    const int n = a.n_coef * a.tp;
    const float* src = a.window + (size_t)s * n;
    if constexpr (PLANES) {
        const int m = a.T * a.n_coef, pp = m + 2 * kHalo;
        float* dst = a.slots + (size_t)b * pp;
        for (int e = threadIdx.x; e < pp; e += 256) {
            const int o = e - kHalo;
            float v = 0.f;
            if (o >= 0 && o < m) {
                const int t = o / a.n_coef, c = o - t * a.n_coef;
                v = src[(size_t)c * a.tp + kHalo + t];
            }
            dst[e] = v;
        }
    } else {
        float* dst = a.slots + (size_t)b * n;
        if (a.vec) {
            const float4* src4 = reinterpret_cast<const float4*>(src);
            float4* dst4 = reinterpret_cast<float4*>(dst);
            for (int e = threadIdx.x; e < n / 4; e += 256) dst4[e] = src4[e];
        } else {
            for (int e = threadIdx.x; e < n; e += 256) dst[e] = src[e];
        }
    }
}

struct StreamMergeArgs {
    const float* c_logits;      // [n][C]: the network's rows, in `selected`'s order
    const float* c_probs;
    const float* f_logits;      // [S][C]: the fill rows (null when n == S)
    const float* f_probs;
    const int64_t* selected;    // [n], strictly increasing
    float* logits;              // [S][C]
    float* probs;
    int S, C, n;
};

// A lane per (stream, class), 256 / C streams per workgroup.  The stream's first lane finds its slot: the first b with selected[b] >= s
// is its slot when selected[b] == s, and it has none otherwise.
__global__ __launch_bounds__(256) void stream_merge_kernel(const StreamMergeArgs a) {
    __shared__ int s_slot[256];
    const int C = a.C, per = 256 / C;
    const int ls = threadIdx.x / C, c = threadIdx.x - ls * C;
    const int s = blockIdx.x * per + ls;
    const bool live = ls < per && s < a.S;
    if (live && c == 0) {
        int lo = 0, hi = a.n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.selected[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        s_slot[ls] = lo < a.n && a.selected[lo] == s ? lo : -1;
    }
    __syncthreads();
    if (!live) return;
    const int slot = s_slot[ls];
    const size_t sc = (size_t)s * C + c;
    if (slot >= 0) {
        const size_t bc = (size_t)slot * C + c;
        a.logits[sc] = a.c_logits[bc];
        a.probs[sc] = a.c_probs[bc];
    } else {
        a.logits[sc] = a.f_logits[sc];
        a.probs[sc] = a.f_probs[sc];
    }
}

namespace {

struct SelectedGeom {
    int64_t slots_off, clogits_off, cprobs_off, net_ws_off, ws_floats;
};

SelectedGeom selected_geom(const StreamGeom& g, const tcr_model_ref& m, const ModelIO& io) {
    SelectedGeom q{};
    int64_t o = g.stage_floats;
    q.slots_off = o; o = align64(o + (int64_t)g.S * model_window_floats(io));
    q.clogits_off = o; o = align64(o + (int64_t)g.S * g.classes);
    q.cprobs_off = o; o = align64(o + (int64_t)g.S * g.classes);
    q.net_ws_off = o;
    q.ws_floats = o + (int64_t)(model_workspace_bytes(m, g.S) / sizeof(float));
    return q;
}

size_t stream_select_bytes(int n_streams) {
    const int64_t tiles = ceil_div64(n_streams, kSelTile);
    return (size_t)(round_up64(n_streams, 256) + round_up64((tiles + 1) * 4, 256));
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_stream_select_init(int n_streams, int32_t* since, void* stream) {
    const char* what = "tcr_stream_select_init";
    TCR_REQUIRE(since, "%s: null argument", what);
    TCR_REQUIRE(n_streams > 0, "%s: the number of streams must be positive (got %d)", what, n_streams);
    hipLaunchKernelGGL(stream_since_init_kernel, dim3(ceil_div(n_streams, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), since,
                       n_streams);
    return check_launch("stream_since_init_kernel");
}

extern "C" size_t tcr_stream_select_workspace_bytes(int n_streams) {
    if (n_streams <= 0) {
        set_error("tcr_stream_select_workspace_bytes: the number of streams must be positive (got %d)", n_streams);
        return 0;
    }
    return stream_select_bytes(n_streams);
}

extern "C" int tcr_stream_select(int n_streams, int num_classes, const float* values, const uint8_t* class_mask, float enter, int pad_after,
                                 const uint8_t* reset, int32_t* since, void* workspace, size_t ws_bytes, int64_t* selected,
                                 int64_t* n_selected, uint8_t* mask, void* stream) {
    const char* what = "tcr_stream_select";
    TCR_REQUIRE(values && class_mask && since && workspace && selected && n_selected, "%s: null argument", what);
    TCR_REQUIRE(n_streams > 0, "%s: the number of streams must be positive (got %d)", what, n_streams);
    TCR_REQUIRE(num_classes > 0 && num_classes <= 256, "%s: num_classes %d outside 1..256", what, num_classes);
    TCR_REQUIRE((int64_t)n_streams * num_classes < ((int64_t)1 << 31), "%s: %d streams x %d classes is too large", what, n_streams,
                num_classes);
    TCR_REQUIRE(enter == enter, "%s: enter is NaN", what);
    TCR_REQUIRE(pad_after >= 0, "%s: pad_after must be >= 0 (got %d)", what, pad_after);
    const size_t need = stream_select_bytes(n_streams);
    if (ws_bytes < need) {
        set_error("%s: workspace %zu bytes < %zu for %d streams", what, ws_bytes, need, n_streams);
        return TCR_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    StreamFlagArgs fa{};
    fa.values = values; fa.class_mask = class_mask; fa.reset = reset; fa.since = since; fa.bits = static_cast<uint8_t*>(workspace);
    fa.mask = mask; fa.S = n_streams; fa.C = num_classes; fa.pad_after = pad_after; fa.enter = enter;
    hipLaunchKernelGGL(stream_flag_kernel, dim3(ceil_div(n_streams, 256 / num_classes)), dim3(256), 0, s, fa);
    TCR_TRY(check_launch("stream_flag_kernel"));
    SelectArgs a{};
    a.bits = fa.bits;
    a.sums = reinterpret_cast<int32_t*>(a.bits + round_up64(n_streams, 256));
    a.selected = selected; a.n_selected = n_selected; a.total = n_streams; a.tiles = (int)ceil_div64(n_streams, kSelTile);
    hipLaunchKernelGGL(select_count_kernel, dim3(a.tiles), dim3(256), 0, s, a);
    TCR_TRY(check_launch("select_count_kernel"));
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, s, a);
    TCR_TRY(check_launch("select_scan_kernel"));
    hipLaunchKernelGGL(select_compact_kernel, dim3(a.tiles), dim3(256), 0, s, a);
    return check_launch("select_compact_kernel");
}

extern "C" size_t tcr_stream_selected_workspace_bytes_m(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int n_streams, int k) {
    const char* what = "tcr_stream_selected_workspace_bytes_m";
    ModelIO io;
    if (stream_check(cfg, model, n_streams, k, nullptr, what, io) != TCR_OK) return 0;
    const StreamGeom g = stream_geom(*cfg, *model, io, n_streams, k, 1);
    return (size_t)selected_geom(g, *model, io).ws_floats * sizeof(float);
}

extern "C" int tcr_stream_step_selected_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams, int k,
                                          const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state, void* workspace,
                                          size_t ws_bytes, const int64_t* selected, int64_t n_selected, const float* fill_logits,
                                          const float* fill_probs, float* logits, float* probs, float* smoothed, int32_t* top, float* score,
                                          int32_t* is_new, void* stream) {
    const char* what = "tcr_stream_step_selected_m";
    const tcr_model_ref* m = model;
    TCR_REQUIRE(plan_dev && m && m->params && m->aux && det && samples && state && workspace && logits && probs && smoothed && top && score &&
                is_new, "%s: null argument", what);
    ModelIO io;
    TCR_TRY(stream_check(cfg, m, n_streams, k, det, what, io));
    TCR_REQUIRE(n_selected >= 0 && n_selected <= n_streams, "%s: n_selected %lld outside 0..%d", what, (long long)n_selected, n_streams);
    TCR_REQUIRE(n_selected == 0 || selected, "%s: null selected with n_selected = %lld", what, (long long)n_selected);
    TCR_REQUIRE(n_selected == n_streams || (fill_logits && fill_probs), "%s: null fill rows with %lld of %d streams selected", what,
                (long long)n_selected, n_streams);
    const StreamGeom g = stream_geom(*cfg, *m, io, n_streams, k, det->average_steps);
    const SelectedGeom q = selected_geom(g, *m, io);
    if ((size_t)q.ws_floats * sizeof(float) > ws_bytes) {
        set_error("%s: workspace %zu bytes < required %zu", what, ws_bytes, (size_t)q.ws_floats * sizeof(float));
        return TCR_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* st = static_cast<float*>(state);
    float* ws = static_cast<float*>(workspace);
    const int n = (int)n_selected;
    const StageArgs sa = stage_args(g, *cfg, samples, reset, st, ws);
    hipLaunchKernelGGL(stream_stage_kernel, dim3(g.S), dim3(256), 0, s, sa);
    TCR_TRY(check_launch("stream_stage_kernel"));
    TCR_TRY(stream_frontend(*cfg, plan_dev, ws, g.stage_stride, g.S, k, st + g.win_off, s));
    float* net_ws = ws + q.net_ws_off;
    const size_t net_bytes = ws_bytes - (size_t)q.net_ws_off * sizeof(float);
    if (n == g.S) {             // tcr_stream_step_m's launches: the state's windows, the caller's rows
        const float* x = st + g.win_off;
        if (io.planes) {
            TCR_TRY(tcr_g2d_input_from_features(x, g.S, g.T, g.n_coef, ws + q.slots_off, stream));
            x = ws + q.slots_off;
        }
        TCR_TRY(model_forward(*m, x, g.S, net_ws, net_bytes, logits, probs, stream));
    } else {
        if (n > 0) {
            StreamGatherArgs ga{};
            ga.window = st + g.win_off; ga.selected = selected; ga.slots = ws + q.slots_off;
            ga.S = g.S; ga.n_coef = g.n_coef; ga.tp = g.tp; ga.T = g.T;
            ga.vec = (g.n_coef * g.tp) % 4 == 0 && ((reinterpret_cast<uintptr_t>(ga.window) | reinterpret_cast<uintptr_t>(ga.slots)) & 15) == 0;
            if (io.planes) hipLaunchKernelGGL(stream_gather_kernel<true>, dim3(n), dim3(256), 0, s, ga);
            else hipLaunchKernelGGL(stream_gather_kernel<false>, dim3(n), dim3(256), 0, s, ga);
            TCR_TRY(check_launch("stream_gather_kernel"));
            TCR_TRY(model_forward(*m, ga.slots, n, net_ws, net_bytes, ws + q.clogits_off, ws + q.cprobs_off, stream));
        }
        StreamMergeArgs ma{};
        ma.c_logits = ws + q.clogits_off; ma.c_probs = ws + q.cprobs_off; ma.f_logits = fill_logits; ma.f_probs = fill_probs;
        ma.selected = selected; ma.logits = logits; ma.probs = probs; ma.S = g.S; ma.C = g.classes; ma.n = n;
        hipLaunchKernelGGL(stream_merge_kernel, dim3(ceil_div(g.S, 256 / g.classes)), dim3(256), 0, s, ma);
        TCR_TRY(check_launch("stream_merge_kernel"));
    }
    DetectArgs da;
    da.probs = probs; da.reset = reset; da.ring = st + g.ring_off; da.ist = reinterpret_cast<int*>(st + g.ist_off);
    da.smoothed = smoothed; da.top = top; da.score = score; da.is_new = is_new;
    da.S = g.S; da.C = g.classes; da.W = g.W; da.min_count = det->min_count; da.suppression = det->suppression_steps; da.threshold = det->threshold;
    hipLaunchKernelGGL(stream_detect_kernel, dim3(ceil_div(g.S, 256 / g.classes)), dim3(256), 0, s, da);
    return check_launch("stream_detect_kernel");
}
