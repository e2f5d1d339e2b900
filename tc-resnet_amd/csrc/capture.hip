// Capturing detections' audio on live streams (tcr_capture_state_bytes / _workspace_bytes / _init / _push / _push_ragged / _flush): a
// recorder next to a streaming detector that hands back, for every detection, the clip tcr_mine_gather would cut from the stream's
// whole recording -- from a ring of the stream's last samples, however the stream is cut into pushes.  The definition (recording,
// trigger, clip, the delay D, the ring length) is include/tcresnet_hip.h's.
//
// The timeline of a call.  Position 0 is the stream's first sample of the call; positions -hist .. -1 are the ring (hist = the samples
// heard since the reset, at most R = the ring's length), position p in ring slot (wpos + p) mod R; positions 0 .. L - 1 are the call's
// samples; everything else is zeros (before the recording's start, and -- tcr_capture_flush only -- audio not yet heard).  The clip of
// trigger row i of a stream whose call starts at its row r0 ends at position (i - r0 + 1) step + lead and is n_samples long, so it is
// at most five stretches of that timeline: zeros, the ring up to its wrap, the ring from slot 0, the call, zeros.
//
// A call (`items`: the call's rows; a flush: the D tail slots of every stream):
//   capture_flag_kernel     a byte per item: row j emits the trigger of row j - D, from the call's rows or the carried tail (dropped by
//                           a reset).  The thread of a stream's first row also copies the stream's (rows, wpos) -- zeros after a reset --
//                           into the workspace: every later kernel of the call reads that copy, so the append may move the state's own;
//   select_count_kernel, select_scan_kernel (scan_select.hip), capture_emit_kernel (select_compact_kernel's positions): the clip table
//                           (stream, row, label, score) in (stream, row) order, the first `capacity` rows, and n_clips;
//   capture_gather_kernel   `parts` workgroups per table row, a grid for min(capacity, items) rows that exits on n_clips: every stretch
//                           through mine.hip's mine_gather_row (16-byte stores fed by aligned 16-byte loads whatever the offsets, and
//                           mine_pcm for the int16 rows: one rounding for mined and captured clips);
//   capture_append_kernel   behind the gather, a thread per 4 (VEC) or 1 of the call's samples: the last R samples of every stream into
//                           its ring; the thread of a stream's last sample moves rows and wpos and rolls the trigger tail.
// tcr_capture_flush runs the same flag / compaction / gather over the tail slots and then capture_clear_kernel.
// No workgroup waits for another (every dependence is a kernel boundary) and no output position comes from an atomic.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after mine.hip).
#pragma once
#include <algorithm>

namespace tcr {

struct alignas(16) CaptureMeta {
    int64_t rows;               // rows heard since the start or the last reset
    int32_t wpos, pad;          // the ring slot of the next sample
};

enum { kCapDense = 0, kCapRagged = 1, kCapFlush = 2 };

struct CaptureArgs {
    const float* samples;       // the call's samples, packed by stream
    const int32_t* top;         // [items]
    const float* score;
    const int32_t* is_new;
    const uint8_t* class_mask;  // [C] or null
    const uint8_t* reset;       // [S] or null (a flush: the streams to flush)
    const int64_t* step_off;    // ragged: [S + 1]
    CaptureMeta* meta;          // state: [S]
    int32_t* tail_flag;         // state: [S][D]: the triggers of the stream's last D rows, the oldest first
    int32_t* tail_label;
    float* tail_score;
    float* ring;                // state: [S][R]
    uint8_t* bits;              // workspace: [items]
    int32_t* sums;              // workspace: [tiles + 1]
    CaptureMeta* snap;          // workspace: [items]; a stream's copy at its first item
    float* out;                 // [capacity][n] or null
    int16_t* out_pcm;
    int32_t* clip_stream;
    int64_t* clip_step;
    int32_t* clip_label;
    float* clip_score;
    int32_t* n_clips;           // [2]: written, due
    int64_t items, steps, capacity, total_samples;      // steps: a dense call's rows per stream (a flush: D)
    int S, C, step, n, lead, D, R, parts, tiles;
};

// item p: its stream, its index among the stream's items of the call, and the stream's first item
template <int MODE>
__device__ __forceinline__ int capture_item(const CaptureArgs& a, int64_t p, int64_t& j, int64_t& first) {
    int s;
    if constexpr (MODE == kCapRagged) {
        s = ragged_signal(a.step_off, a.S, p);
        first = a.step_off[s];
    } else {
        s = (int)(p / a.steps);
        first = (int64_t)s * a.steps;
    }
    j = p - first;
    return s;
}

// row q of the call is a trigger
__device__ __forceinline__ bool capture_trigger(const CaptureArgs& a, int64_t q) {
    if (a.is_new[q] == 0) return false;
    if (!a.class_mask) return true;
    const int c = a.top[q];
    return c >= 0 && c < a.C && a.class_mask[c] != 0;
}

template <int MODE>
__global__ __launch_bounds__(256) void capture_flag_kernel(const CaptureArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.items) return;
    int64_t j, first;
    const int s = capture_item<MODE>(a, p, j, first);
    bool f;
    if constexpr (MODE == kCapFlush) {
        f = (!a.reset || a.reset[s] != 0) && a.tail_flag[(int64_t)s * a.D + j] != 0;
    } else {
        const bool fresh = a.reset && a.reset[s] != 0;
        if (j == 0) a.snap[first] = fresh ? CaptureMeta{0, 0, 0} : a.meta[s];
        if (j >= a.D) f = capture_trigger(a, p - a.D);
        else f = !fresh && a.tail_flag[(int64_t)s * a.D + j] != 0;
    }
    a.bits[p] = f ? 1 : 0;
}

// select_compact_kernel's positions over the items' flags; the first `capacity` clips' table rows, and the two counts.
template <int MODE>
__global__ __launch_bounds__(256) void capture_emit_kernel(const SelectArgs sa, const CaptureArgs a) {
    int v[4], total;
    const int64_t at = select_tile_bits(sa, v);
    int64_t out = sa.sums[blockIdx.x] + select_block_prefix(v[0] + v[1] + v[2] + v[3], total);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int64_t due = sa.sums[sa.tiles];
        a.n_clips[0] = (int32_t)(due < a.capacity ? due : a.capacity);
        a.n_clips[1] = (int32_t)due;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (!v[e]) continue;
        if (out < a.capacity) {
            const int64_t p = at + e;
            int64_t j, first;
            const int s = capture_item<MODE>(a, p, j, first);
            const int64_t base = MODE == kCapFlush ? a.meta[s].rows : a.snap[first].rows;
            a.clip_stream[out] = s;
            a.clip_step[out] = base + j - a.D;
            if (MODE != kCapFlush && j >= a.D) {
                a.clip_label[out] = a.top[p - a.D];
                a.clip_score[out] = a.score[p - a.D];
            } else {
                a.clip_label[out] = a.tail_label[(int64_t)s * a.D + j];
                a.clip_score[out] = a.tail_score[(int64_t)s * a.D + j];
            }
        }
        ++out;
    }
}

// d[e0 .. e0 + cnt) of both outputs <- src[first .. first + cnt) of a stretch of len samples (len 0: zeros)
__device__ __forceinline__ void capture_stretch(const CaptureArgs& a, int64_t i, const float* src, int64_t len, int64_t first, int64_t e0,
                                                int64_t cnt, int part) {
    if (cnt <= 0) return;
    if (a.out) mine_gather_row(src, len, first, a.out + i * a.n + e0, (int)cnt, part, a.parts);
    if (a.out_pcm) mine_gather_row(src, len, first, a.out_pcm + i * a.n + e0, (int)cnt, part, a.parts);
}

__device__ __forceinline__ int64_t capture_min(int64_t x, int64_t y) { return x < y ? x : y; }
__device__ __forceinline__ int64_t capture_max(int64_t x, int64_t y) { return x > y ? x : y; }

// clip i of the table, this workgroup's part of it
template <int MODE>
__device__ __forceinline__ void capture_gather_clip(const CaptureArgs& a, int64_t i, int part) {
    const int s = a.clip_stream[i];
    CaptureMeta m;
    const float* call = a.ring;
    int64_t L = 0;
    if constexpr (MODE == kCapFlush) {
        m = a.meta[s];
    } else {
        int64_t first, rows;
        if constexpr (MODE == kCapRagged) {
            first = a.step_off[s];
            rows = a.step_off[s + 1] - first;
        } else {
            first = (int64_t)s * a.steps;
            rows = a.steps;
        }
        m = a.snap[first];
        call = a.samples + first * a.step;
        L = rows * a.step;
    }
    const int64_t heard = m.rows * a.step, hist = heard < a.R ? heard : a.R;
    const int64_t t1 = (a.clip_step[i] - m.rows + 1) * a.step + a.lead, t0 = t1 - a.n;
    const float* ring = a.ring + (int64_t)s * a.R;
    // zeros before the recording's start (or before what the ring still holds: never reached, see the header)
    int64_t q0 = t0, q1 = capture_min(t1, -hist);
    capture_stretch(a, i, ring, 0, 0, 0, q1 - q0, part);
    // the ring, in at most two stretches
    q0 = capture_max(t0, -hist);
    q1 = capture_min(t1, 0);
    if (q1 > q0) {
        int64_t slot = (m.wpos + q0) % a.R;
        if (slot < 0) slot += a.R;
        const int64_t n0 = capture_min(q1 - q0, a.R - slot);
        capture_stretch(a, i, ring, a.R, slot, q0 - t0, n0, part);
        capture_stretch(a, i, ring, a.R, 0, q0 - t0 + n0, q1 - q0 - n0, part);
    }
    // the call's samples
    q0 = capture_max(t0, 0);
    q1 = capture_min(t1, L);
    capture_stretch(a, i, call, L, q0, q0 - t0, q1 - q0, part);
    // audio not yet heard (a flush)
    q0 = capture_max(t0, L);
    capture_stretch(a, i, ring, 0, 0, q0 - t0, t1 - q0, part);
}

// `parts` workgroups per clip the call can write; nothing past the device-side count.
template <int MODE>
__global__ __launch_bounds__(256) void capture_gather_kernel(const CaptureArgs a) {
    const int64_t i = blockIdx.x / (unsigned)a.parts;
    if (i < a.n_clips[0]) capture_gather_clip<MODE>(a, i, (int)(blockIdx.x - (unsigned)i * a.parts));
}

// A thread per W = 4 (VEC: step, R and both bases keep every position 16-byte aligned) or 1 of the call's samples.
template <bool RAGGED, bool VEC>
__global__ __launch_bounds__(256) void capture_append_kernel(const CaptureArgs a) {
    constexpr int W = VEC ? 4 : 1;
    const int64_t x = ((int64_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (x >= a.total_samples) return;
    int s;
    int64_t first, rows;
    if constexpr (RAGGED) {
        s = ragged_signal(a.step_off, a.S, x / a.step);
        first = a.step_off[s];
        rows = a.step_off[s + 1] - first;
    } else {
        s = (int)(x / (a.steps * a.step));
        first = (int64_t)s * a.steps;
        rows = a.steps;
    }
    const int64_t L = rows * a.step, p = x - first * a.step;
    const CaptureMeta m = a.snap[first];
    if (p >= L - a.R) {
        float* d = a.ring + (int64_t)s * a.R + (m.wpos + p) % a.R;
        if constexpr (VEC) *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(a.samples + x);
        else *d = a.samples[x];
    }
    if (p + W != L) return;
    // the stream's last sample: the state's integers and the tail, read only by the kernels in front of this one
    a.meta[s] = CaptureMeta{m.rows + rows, (int32_t)((m.wpos + L) % a.R), 0};
    const bool fresh = a.reset && a.reset[s] != 0;
    const int64_t t = (int64_t)s * a.D;
    for (int k = 0; k < a.D; ++k) {                     // (in place: slot k reads slot k + rows > k, or the call)
        const int64_t src = rows - a.D + k;
        int f = 0, label = 0;
        float sc = 0.f;
        if (src >= 0) {
            f = capture_trigger(a, first + src);
            if (f) { label = a.top[first + src]; sc = a.score[first + src]; }
        } else if (!fresh && a.tail_flag[t + k + rows] != 0) {
            f = 1; label = a.tail_label[t + k + rows]; sc = a.tail_score[t + k + rows];
        }
        a.tail_flag[t + k] = f;
        a.tail_label[t + k] = label;
        a.tail_score[t + k] = sc;
    }
}

// a flush: the flushed streams' triggers are gone
__global__ __launch_bounds__(256) void capture_clear_kernel(const CaptureArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= a.items) return;
    if (a.reset && a.reset[p / a.D] == 0) return;
    a.tail_flag[p] = 0;
    a.tail_label[p] = 0;
    a.tail_score[p] = 0.f;
}

__global__ void capture_none_kernel(int32_t* n_clips) { n_clips[0] = n_clips[1] = 0; }

namespace {

struct CaptureGeom {
    int D;                      // rows between a trigger and the call that emits its clip
    int R;                      // the ring's samples: n_samples + max(0, -lead), rounded up to 4
    size_t tail_off, ring_off, bytes;
};

// | meta [S] | tail_flag, tail_label, tail_score [S][D] | ring [S][R] |, each rounded up to 256 bytes
int capture_geom(const char* what, int S, int step, int n, int lead, CaptureGeom& g) {
    TCR_REQUIRE(S > 0, "%s: the number of streams must be positive (got %d)", what, S);
    TCR_REQUIRE(step > 0, "%s: step_samples must be positive (got %d)", what, step);
    TCR_REQUIRE(n > 0, "%s: n_samples must be positive (got %d)", what, n);
    constexpr int kMax = 1 << 28;
    TCR_REQUIRE(step <= kMax && n <= kMax && lead >= -kMax && lead <= kMax, "%s: step_samples %d, n_samples %d or lead %d outside +-2^28", what,
                step, n, lead);
    g.D = lead > 0 ? (int)ceil_div64(lead, step) : 0;
    g.R = (int)round_up64((int64_t)n + (lead < 0 ? -(int64_t)lead : 0), 4);
    const double need = (double)S * (16.0 + 12.0 * g.D + 4.0 * g.R);
    TCR_REQUIRE(need < 1e15, "%s: size overflow: %d streams with a ring of %d samples and %d pending rows need %.3g bytes", what, S, g.R, g.D,
                need);
    g.tail_off = (size_t)round_up64((int64_t)S * (int64_t)sizeof(CaptureMeta), 256);
    g.ring_off = g.tail_off + (size_t)round_up64((int64_t)S * g.D * 12, 256);
    g.bytes = g.ring_off + (size_t)S * g.R * sizeof(float);
    return TCR_OK;
}

// the workspace of `items` items: bits | sums | snap
struct CaptureWs {
    size_t sums_off, snap_off, bytes;
};

CaptureWs capture_ws(int64_t items) {
    CaptureWs w;
    w.sums_off = (size_t)round_up64(items, 256);
    w.snap_off = w.sums_off + (size_t)round_up64((ceil_div64(items, kSelTile) + 1) * 4, 256);
    w.bytes = w.snap_off + (size_t)items * sizeof(CaptureMeta);
    return w;
}

struct CaptureOut {
    float* out;
    int16_t* out_pcm;
    int32_t* clip_stream;
    int64_t* clip_step;
    int32_t* clip_label;
    float* clip_score;
    int32_t* n_clips;
};

// the checks and pointers every call shares
int capture_args(const char* what, int S, int step, int n, int lead, void* state, void* workspace, size_t ws_bytes, int64_t items,
                 int64_t capacity, const CaptureOut& o, CaptureArgs& a, CaptureGeom& g) {
    TCR_TRY(capture_geom(what, S, step, n, lead, g));
    TCR_REQUIRE(state && o.n_clips, "%s: null argument", what);
    TCR_REQUIRE((reinterpret_cast<uintptr_t>(state) & 15) == 0, "%s: the state must be 16-byte aligned", what);
    TCR_REQUIRE(capacity >= 0 && capacity < ((int64_t)1 << 31), "%s: capacity %lld outside 0..2^31 - 1", what, (long long)capacity);
    TCR_REQUIRE(capacity == 0 || (o.clip_stream && o.clip_step && o.clip_label && o.clip_score), "%s: null clip tables with capacity %lld", what,
                (long long)capacity);
    char* st = static_cast<char*>(state);
    a.meta = reinterpret_cast<CaptureMeta*>(st);
    a.tail_flag = reinterpret_cast<int32_t*>(st + g.tail_off);
    a.tail_label = a.tail_flag + (int64_t)S * g.D;
    a.tail_score = reinterpret_cast<float*>(a.tail_label + (int64_t)S * g.D);
    a.ring = reinterpret_cast<float*>(st + g.ring_off);
    a.out = o.out; a.out_pcm = o.out_pcm; a.clip_stream = o.clip_stream; a.clip_step = o.clip_step; a.clip_label = o.clip_label;
    a.clip_score = o.clip_score; a.n_clips = o.n_clips;
    a.capacity = capacity; a.S = S; a.step = step; a.n = n; a.lead = lead; a.D = g.D; a.R = g.R;
    a.parts = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div64(n, 4 * 256 * 4), 64));
    a.items = items;
    if (items > 0) {
        TCR_REQUIRE(items < ((int64_t)1 << 31), "%s: %lld rows in a call, at most 2^31 - 1", what, (long long)items);
        TCR_REQUIRE(workspace, "%s: null argument", what);
        TCR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
        const CaptureWs w = capture_ws(items);
        if (ws_bytes < w.bytes) {
            set_error("%s: workspace %zu bytes < %zu for %lld rows", what, ws_bytes, w.bytes, (long long)items);
            return TCR_ERR_WORKSPACE;
        }
        char* ws = static_cast<char*>(workspace);
        a.bits = reinterpret_cast<uint8_t*>(ws);
        a.sums = reinterpret_cast<int32_t*>(ws + w.sums_off);
        a.snap = reinterpret_cast<CaptureMeta*>(ws + w.snap_off);
        a.tiles = (int)ceil_div64(items, kSelTile);
        TCR_REQUIRE(std::min(capacity, items) * a.parts < ((int64_t)1 << 31), "%s: %lld clips of %d samples are too many for one launch", what,
                    (long long)std::min(capacity, items), n);
    }
    return TCR_OK;
}

// flag, compaction and gather over a.items items
template <int MODE>
int capture_emit(const CaptureArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(capture_flag_kernel<MODE>, dim3((unsigned)ceil_div64(a.items, 256)), dim3(256), 0, s, a);
    TCR_TRY(check_launch("capture_flag_kernel"));
    SelectArgs sa{};
    sa.bits = a.bits; sa.sums = a.sums; sa.total = a.items; sa.tiles = a.tiles;
    hipLaunchKernelGGL(select_count_kernel, dim3(sa.tiles), dim3(256), 0, s, sa);
    TCR_TRY(check_launch("select_count_kernel"));
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, s, sa);
    TCR_TRY(check_launch("select_scan_kernel"));
    hipLaunchKernelGGL(capture_emit_kernel<MODE>, dim3(sa.tiles), dim3(256), 0, s, sa, a);
    TCR_TRY(check_launch("capture_emit_kernel"));
    // (a grid for every clip the call can write: bounding it at eight workgroups a compute unit and walking the rest by stride left the
    // empty push where it was and cost 15 % with every stream triggering, OPTLOG.md)
    const int64_t rows = std::min(a.capacity, a.items);
    if (rows > 0 && (a.out || a.out_pcm)) {
        hipLaunchKernelGGL(capture_gather_kernel<MODE>, dim3((unsigned)(rows * a.parts)), dim3(256), 0, s, a);
        TCR_TRY(check_launch("capture_gather_kernel"));
    }
    return TCR_OK;
}

int capture_push(const char* what, bool ragged, int S, int64_t steps, const int64_t* step_offsets, int64_t total_steps, int step, int n,
                 int lead, const float* samples, const int32_t* top, const float* score, const int32_t* is_new, const uint8_t* class_mask,
                 int num_classes, const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, int64_t capacity, const CaptureOut& o,
                 void* stream) {
    TCR_REQUIRE((!ragged || step_offsets) && samples && top && score && is_new, "%s: null argument", what);
    TCR_REQUIRE(ragged ? total_steps > 0 : steps > 0, "%s: the number of steps must be positive (got %lld)", what,
                (long long)(ragged ? total_steps : steps));
    TCR_REQUIRE(!class_mask || num_classes > 0, "%s: a class mask over %d classes", what, num_classes);
    TCR_REQUIRE(S > 0, "%s: the number of streams must be positive (got %d)", what, S);
    TCR_REQUIRE(steps < ((int64_t)1 << 31), "%s: %lld rows in a call, at most 2^31 - 1", what, (long long)steps);
    const int64_t items = ragged ? total_steps : steps * S;
    CaptureArgs a{};
    CaptureGeom g;
    TCR_TRY(capture_args(what, S, step, n, lead, state, workspace, ws_bytes, items, capacity, o, a, g));
    a.total_samples = items * step;
    TCR_REQUIRE(a.total_samples < ((int64_t)1 << 40), "%s: %lld samples in a call, at most 2^40 - 1", what, (long long)a.total_samples);
    a.samples = samples; a.top = top; a.score = score; a.is_new = is_new; a.class_mask = class_mask; a.C = num_classes; a.reset = reset;
    a.step_off = ragged ? step_offsets : nullptr;
    a.steps = ragged ? 0 : steps;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TCR_TRY(ragged ? capture_emit<kCapRagged>(a, s) : capture_emit<kCapDense>(a, s));
    const bool vec = step % 4 == 0 && (reinterpret_cast<uintptr_t>(samples) & 15) == 0;         // (R is a multiple of 4, the ring 16-byte aligned)
    const auto append = ragged ? (vec ? capture_append_kernel<true, true> : capture_append_kernel<true, false>)
                               : (vec ? capture_append_kernel<false, true> : capture_append_kernel<false, false>);
    hipLaunchKernelGGL(append, dim3((unsigned)ceil_div64(a.total_samples, vec ? 1024 : 256)), dim3(256), 0, s, a);
    return check_launch("capture_append_kernel");
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" size_t tcr_capture_state_bytes(int n_streams, int step_samples, int n_samples, int lead) {
    CaptureGeom g;
    if (capture_geom("tcr_capture_state_bytes", n_streams, step_samples, n_samples, lead, g) != TCR_OK) return 0;
    return g.bytes;
}

extern "C" size_t tcr_capture_workspace_bytes(int64_t total_rows) {
    if (total_rows <= 0 || total_rows >= ((int64_t)1 << 31)) {
        set_error("tcr_capture_workspace_bytes: total_rows %lld outside 1..2^31 - 1", (long long)total_rows);
        return 0;
    }
    return capture_ws(total_rows).bytes;
}

extern "C" int tcr_capture_init(int n_streams, int step_samples, int n_samples, int lead, void* state, void* stream) {
    const char* what = "tcr_capture_init";
    CaptureGeom g;
    TCR_TRY(capture_geom(what, n_streams, step_samples, n_samples, lead, g));
    TCR_REQUIRE(state, "%s: null argument", what);
    // (the ring's slots are written before they are read; zeros keep the state's bytes defined)
    if (hipMemsetAsync(state, 0, g.bytes, static_cast<hipStream_t>(stream)) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", what);
        return TCR_ERR_HIP;
    }
    return TCR_OK;
}

extern "C" int tcr_capture_push(int n_streams, int64_t steps, int step_samples, int n_samples, int lead, const float* samples,
                                const int32_t* top, const float* score, const int32_t* is_new, const uint8_t* class_mask, int num_classes,
                                const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, int64_t capacity, float* out,
                                int16_t* out_pcm, int32_t* clip_stream, int64_t* clip_step, int32_t* clip_label, float* clip_score,
                                int32_t* n_clips, void* stream) {
    return capture_push("tcr_capture_push", false, n_streams, steps, nullptr, 0, step_samples, n_samples, lead, samples, top, score, is_new,
                        class_mask, num_classes, reset, state, workspace, ws_bytes, capacity,
                        CaptureOut{out, out_pcm, clip_stream, clip_step, clip_label, clip_score, n_clips}, stream);
}

extern "C" int tcr_capture_push_ragged(int n_streams, const int64_t* step_offsets, int64_t total_steps, int step_samples, int n_samples,
                                       int lead, const float* samples, const int32_t* top, const float* score, const int32_t* is_new,
                                       const uint8_t* class_mask, int num_classes, const uint8_t* reset, void* state, void* workspace,
                                       size_t ws_bytes, int64_t capacity, float* out, int16_t* out_pcm, int32_t* clip_stream,
                                       int64_t* clip_step, int32_t* clip_label, float* clip_score, int32_t* n_clips, void* stream) {
    return capture_push("tcr_capture_push_ragged", true, n_streams, 0, step_offsets, total_steps, step_samples, n_samples, lead, samples, top,
                        score, is_new, class_mask, num_classes, reset, state, workspace, ws_bytes, capacity,
                        CaptureOut{out, out_pcm, clip_stream, clip_step, clip_label, clip_score, n_clips}, stream);
}

extern "C" int tcr_capture_flush(int n_streams, const uint8_t* mask, int step_samples, int n_samples, int lead, void* state, void* workspace,
                                 size_t ws_bytes, int64_t capacity, float* out, int16_t* out_pcm, int32_t* clip_stream, int64_t* clip_step,
                                 int32_t* clip_label, float* clip_score, int32_t* n_clips, void* stream) {
    const char* what = "tcr_capture_flush";
    CaptureGeom g;
    TCR_TRY(capture_geom(what, n_streams, step_samples, n_samples, lead, g));
    CaptureArgs a{};
    TCR_TRY(capture_args(what, n_streams, step_samples, n_samples, lead, state, workspace, ws_bytes, (int64_t)n_streams * g.D, capacity,
                         CaptureOut{out, out_pcm, clip_stream, clip_step, clip_label, clip_score, n_clips}, a, g));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a.items == 0) {                                 // lead <= 0: nothing is ever pending
        hipLaunchKernelGGL(capture_none_kernel, dim3(1), dim3(1), 0, s, n_clips);
        return check_launch("capture_none_kernel");
    }
    a.reset = mask;
    a.steps = g.D;
    TCR_TRY(capture_emit<kCapFlush>(a, s));
    hipLaunchKernelGGL(capture_clear_kernel, dim3((unsigned)ceil_div64(a.items, 256)), dim3(256), 0, s, a);
    return check_launch("capture_clear_kernel");
}
