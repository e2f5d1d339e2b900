// Many detector steps in one call, over one chunk pipeline with three compile-time axes:
//   CARRIED  the call starts from the stream state of stream.hip and writes it back (tcr_stream_scan, tcr_stream_scan_ragged: bitwise
//            that many calls of tcr_stream_step, outputs and state) or starts fresh and writes nothing back (tcr_scan, tcr_scan_ragged:
//            every step of N recordings, bitwise what a fresh streaming detector returns push by push).  The state (ScanState) is the
//            pipeline's variable part, and "fresh" is what reset[s] != 0 means as well;
//   RAGGED   every signal (stream) brings its own number of steps, packed one after the other (the _ragged entries), or all bring the
//            same number (dense);
//   PLANES   the windows are the 2-D graph's [T x n_coef] planes or planar [n_coef][T + 2 TCR_HALO].
//
// In frames of  x = tail ++ samples  (the stream's tail, zeros when fresh, then the call's L = m k hop samples), new frame j covers
// x[j hop, j hop + win): the samples tcr_stream_step's staging rows hold for the same frame, and a frame is a pure function of its
// samples (frontend_pk3.hip).  Column t of step i's window is new frame (i + 1) k - T + t; a negative index -e is column T - e of the
// carried window.  For a fresh signal the frames of negative index cover zeros only and are computed like any other frame, which is
// how the zero window itself was computed, so its windows need no carried column.  The network's result for a window does not depend
// on its batch (DESIGN, net_small_tc8_kernel), the smoothing of step i reads the probabilities of steps i - W + 1 .. i only, and the
// suppression state changes only at candidate steps (count >= min_count && score > threshold).  So the windows are computed at the
// network's batch throughput and only the suppression is sequential.
//
// Steps are cut into groups of G consecutive steps of one signal; a group is one front-end row of F = G k + T - k frames from new frame
// g G k + k - T on.  The groups are flattened over the signals in order (dense: signal q / groups, group q % groups; ragged: the prefix
// table group_off), and a chunk is R consecutive groups:
//   staging               the R rows (tail ++ samples, zeros outside): scan_stage_kernel, a thread per sample, or
//                         scan_stage_ragged_kernel<CARRIED>, whose workgroups look their row's signal up once;
//   frontend_pk3_kernel   <.., STREAM = true> over R rows of F frames into frame rows [R][n_coef][F + 2 TCR_HALO] (column 0 on);
//   scan_gather_kernel    <PLANES, CARRIED, RAGGED>: the windows from the frame rows, or from carried columns for negative frames,
//                         [slots][n_coef][T + 2 TCR_HALO] (zero halo) or the planes [slots][1][T n_coef + 2 TCR_HALO];
//   scan_carry_kernel     <PLANES, RAGGED>, with a state: window and tail write-back of the streams whose last group is in this chunk;
//   the network at the batch of the slots (detect_model.h: tcr_net_forward_frozen, tcr_dscnn_forward_infer or tcr_g2d_forward_infer);
//   scan_scatter_kernel   dense only: logits / probs of the slots that are steps (g G + j < steps) into the caller's [N][steps][C].
// Dense, a chunk has R G slots; those past a signal's last step (the last group of a signal may be short) are computed and dropped.
// Ragged, a signal's groups cover its steps in order, so a chunk's live steps are one contiguous range of packed steps: the gather
// writes them compactly (slot = p - p(q0)), the network runs at the batch of the live steps and writes their rows of the caller's
// logits / probs itself -- no scatter, and the dead slots of a short last group cost front-end frames only.  Then, once per call:
//   scan_smooth_kernel    <CARRIED, RAGGED>, a lane per (signal, step, class): smoothed over count_i = min(count0 + i + 1, W) vectors,
//                         those of steps before the call from ring slots (head0 - d) mod W, oldest first; top, score and the candidate
//                         flag (is_new = top + 1 or 0);
//   scan_suppress_kernel  <RAGGED>, a workgroup per signal: the ring write-back (the last min(W, m) vectors at slots (head0 + i) mod W:
//                         the smoothing has read the old ones), the detections in step order from the carried prev_label and
//                         prev_step - n0, rewritten into is_new, then the five detector integers.
//
// The ragged tables: step_off [N + 1] (signal n's steps are packed rows step_off[n] ..) and, once G is chosen, group_off [N + 1] (its
// ceil(steps_n / G) groups are flattened rows group_off[n] ..); the host builds both and uploads them to the front of the workspace, and
// the kernels find the signal of a flattened group or a packed step by binary search (ragged_signal).  The smoothing counts from the
// signal's first row and the suppression walks the signal's own rows, so a signal's rows are bitwise its dense scan alone.  The results
// do not depend on G: dense takes balanced groups, ragged the group size with the fewest front-end frames over the call (scan_chunking).
//
// State ordering.  A stream's groups are consecutive flattened rows (dense and ragged), so its window and tail are written only in the
// chunk that holds its last group, after that chunk's stage and gather (the window is its last step's, gathered just before; the tail
// the last tail_len samples of x, the old samples that survive a short call read before it is written), and no later chunk has a group
// of that stream to read them; ring and integers are written by the suppression, after the smoothing of every stream has read them.  A
// stream without steps (m_s == 0, ragged) has no group, no row and no carry, and its suppression workgroup returns before it reads or
// writes anything: its window, tail, ring and five integers are byte for byte what they were -- and so reset[s] != 0 with m_s == 0 is
// ignored (the caller keeps it for the call that brings the stream's next step).
//
// The axes are compile-time instances and not tests at run time because the dense fresh scan pays for such tests: the state test cost
// tcr_scan 5 % of the gather and doubled its smoothing (profiles/scan_unify_kernel_stats.csv), and the dense instances carry no table
// lookup.  The dense staging keeps its thread-per-sample form.
//
// Workspace (tcr_scan_workspace_bytes), regions 256-byte aligned:
//   staging [R][stage_stride] | frame rows [R][n_coef][F + 8] | windows [R G][n_coef][Tp] (2-D graph: planes [R G][T n_coef + 8])
//   | logits, probs [R G][C] | network at R G.
// It does not depend on the signals' length; R and G are derived from the bytes the caller passes.  tcr_scan_ragged_workspace_bytes
// puts the tables [2][max_signals + 1] int64 (rounded up to 256 bytes) in front of it.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after stream.hip).
#pragma once
#include <algorithm>
#include <vector>

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

// The stream state a call starts from and writes back (StreamGeom's regions, stream.hip).  All null: no state, every signal is fresh
// and nothing is written back (tcr_scan).  reset[s] != 0 makes stream s fresh for this call; its state is written all the same.
struct ScanState {
    float* window;              // [S][n_coef][tp]
    float* tail;                // [S][tail_len]
    float* ring;                // [W][S][C]
    int* ist;                   // [5][S]: head, count, prev_label, prev_step, n
    const uint8_t* reset;       // [S] or null
    int tail_len;               // >= 0 (StreamGeom::tail_len)
};

__device__ __forceinline__ bool scan_fresh(const ScanState& st, int64_t s) { return !st.window || (st.reset && st.reset[s]); }

// The detector integers in front of a state of their own (phrase.hip, dtw.hip): [5][S] int32 rounded up to 256 bytes, and entry i of
// them for streams that have seen no rows and have no detection yet (false: i lies behind the integers).
inline size_t detect_state_ints_bytes(int S) { return (size_t)round_up64((int64_t)S * 5 * sizeof(int32_t), 256); }

__device__ __forceinline__ bool detect_ints_init(int* ist, int S, int64_t i) {
    if (i >= 5 * (int64_t)S) return false;
    ist[i] = i / S == 2 ? -1 : 0;
    return true;
}

// a chunk: rows q0 .. q0 + rows - 1 of the call's groups (signal q / groups, group q % groups)
struct ScanChunkArgs {
    const float* samples;       // [N][L]
    float* stage;               // [R][stride]
    float* frames;              // [R][n_coef][ftp]
    float* windows;             // [R G][n_coef][tp] (planes: [R G][T n_coef + 2 kHalo])
    ScanState st;
    int64_t L, stride, q0, rows, groups, steps, n_prefix, k_hop;
    int64_t s0;                 // scan_carry_kernel: the first stream whose last group is in the chunk
    int G, k, T, tp, n_coef, ftp;
    // ragged (tcr_scan_ragged): the prefix tables, and the packed step of the chunk's first slot
    const int64_t* step_off;    // [N + 1]: signal n's steps are packed rows step_off[n] .. step_off[n + 1] - 1
    const int64_t* group_off;   // [N + 1]: its groups are flattened rows group_off[n] .. group_off[n + 1] - 1
    int64_t p0;
    int n_sig;
};

// Ragged index mapping: the signal of packed step (or flattened group) v < off[N] is the last n with off[n] <= v -- a signal without
// steps shares its successor's offset and is never the answer.  A binary search over the table, log2 N reads that every lane of a
// wave shares (the table of a whole evaluation corpus stays in L2).
__device__ __forceinline__ int ragged_signal(const int64_t* off, int n_sig, int64_t v) {
    int lo = 0, hi = n_sig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Staging row r = group q0 + r: x from new frame g G k + k - T on, i.e. from sample (g G + 1) k hop of  zeros(n_prefix) ++ signal ++
// zeros  (n_prefix = the clip's n_samples = T hop + win - hop + remainder), with the stream's tail in the last tail_len samples of the
// prefix.  The rows are placed by sample position, so a hop > win whose steps begin in the gap between two frames (stream.hip:
// tail_len = 0, skip > 0) needs nothing here: every new frame then lies within the call's samples, and no tail is read.
// One thread per staged sample.
__global__ __launch_bounds__(256) void scan_stage_kernel(const ScanChunkArgs a) {
    const int64_t total = a.rows * a.stride;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / a.stride, x = e - r * a.stride;
        const int64_t q = a.q0 + r, n = q / a.groups, g = q - n * a.groups;
        const int64_t pos = (g * a.G + 1) * a.k_hop + x - a.n_prefix;           // sample of the signal; < 0: before the call
        float v = 0.f;
        if (pos >= 0) {
            if (pos < a.L) v = a.samples[n * a.L + pos];
        } else if (pos + a.st.tail_len >= 0 && !scan_fresh(a.st, n)) {
            v = a.st.tail[n * a.st.tail_len + pos + a.st.tail_len];
        }
        a.stage[e] = v;
    }
}

// The ragged staging row: bx workgroups per row, so that the row's signal is looked up once per thread and not once per sample.
// Signal n's samples start at step_off[n] k hop of the packed buffer, with zeros in front and behind.  CARRIED: positions before the
// call come from the last tail_len samples of the prefix, the stream's tail (zeros when it is fresh; with a small G several groups of
// a stream reach into the prefix).
template <bool CARRIED>
__global__ __launch_bounds__(256) void scan_stage_ragged_kernel(const ScanChunkArgs a, const int bx) {
    const int64_t r = blockIdx.x / (unsigned)bx;
    const int part = (int)(blockIdx.x - (unsigned)r * bx);
    const int64_t q = a.q0 + r;
    const int n = ragged_signal(a.group_off, a.n_sig, q);
    const int64_t g = q - a.group_off[n];
    const int64_t first = a.step_off[n], len = (a.step_off[n + 1] - first) * a.k_hop;
    const float* src = a.samples + first * a.k_hop;
    const int tail_len = a.st.tail_len;
    const float* tail = nullptr;                                                // (indexed by pos < 0)
    if constexpr (CARRIED) tail = scan_fresh(a.st, n) ? nullptr : a.st.tail + (size_t)n * tail_len + tail_len;
    const int64_t base = (g * a.G + 1) * a.k_hop - a.n_prefix;
    float* dst = a.stage + r * a.stride;
    for (int64_t x = (int64_t)part * 256 + threadIdx.x; x < a.stride; x += (int64_t)bx * 256) {
        const int64_t pos = base + x;
        float v = 0.f;
        if (pos >= 0) {
            if (pos < len) v = src[pos];
        } else if constexpr (CARRIED) {
            if (tail && pos + tail_len >= 0) v = tail[pos];
        }
        dst[x] = v;
    }
}

// Window slot b of a chunk: its frame row r and step j within the row's group, its signal (stream) s and (i + 1) k of its step i = g G +
// j.  Dense: slot b = r G + j of flattened group q0 + r.  RAGGED: the slots are compact, slot b is packed step p0 + b, and signal, step
// and group come from the prefix tables.
struct ScanSlot {
    int r, j;
    int64_t s, i1;
};

template <bool RAGGED>
__device__ __forceinline__ ScanSlot scan_slot(const ScanChunkArgs& a, int b) {
    ScanSlot o;
    if constexpr (RAGGED) {
        const int64_t p = a.p0 + b;
        const int n = ragged_signal(a.step_off, a.n_sig, p);
        const int64_t i = p - a.step_off[n], g = i / a.G;
        o.j = (int)(i - g * a.G);
        o.r = (int)(a.group_off[n] + g - a.q0);
        o.s = n;
        o.i1 = (i + 1) * a.k;
    } else {
        o.r = b / a.G;
        o.j = b - o.r * a.G;
        const int64_t q = a.q0 + o.r;
        o.s = q / a.groups;
        const int64_t g = q - o.s * a.groups;
        o.i1 = (g * a.G + o.j + 1) * a.k;
    }
    return o;
}

// One workgroup per window slot b (scan_slot): column t is column j k + t of frame row r when new frame (i + 1) k - T + t >= 0 or the
// signal is fresh, else column (i + 1) k + t of the carried window; the halo is zero.  PLANES (2-D graph): the same window as its
// [T x n_coef] plane, written in plane order (coalesced): plane offset t n_coef + c <- window column t, coefficient c
// (features_to_plane_kernel's map, net2d_kernels.hip).  A pure copy: bitwise the planar gather followed by features_to_plane_kernel.
// CARRIED: the call has a state; without one no column is carried, and the instance is the plain copy (the test at run time cost
// tcr_scan 5 % of this kernel, profiles/scan_unify_kernel_stats.csv).  sh is set by a select and the carried pointer unconditionally:
// a nested-if form was compiled wrongly for reset[s] == 0 under a non-null reset array (profiles/scan_unify_kernel_regs.txt).
template <bool PLANES, bool CARRIED, bool RAGGED>
__global__ __launch_bounds__(256) void scan_gather_kernel(const ScanChunkArgs a) {
    const int b = blockIdx.x;
    const ScanSlot sl = scan_slot<RAGGED>(a, b);
    const float* src = a.frames + (size_t)sl.r * a.n_coef * a.ftp + sl.j * a.k;        // window column x <- frame-row column j k + x
    const float* old = src;                                                     // (not read while sh = T)
    int sh = a.T;                                                               // carried columns: t < T - sh
    if constexpr (CARRIED) {
        if (sl.i1 < a.T && !scan_fresh(a.st, sl.s)) sh = (int)sl.i1;
        old = a.st.window + (size_t)sl.s * a.n_coef * a.tp + sh;
    }
    if constexpr (PLANES) {
        const int n = a.T * a.n_coef, pp = n + 2 * kHalo;
        float* dst = a.windows + (size_t)b * pp;
        for (int i = threadIdx.x; i < pp; i += 256) {
            const int o = i - kHalo;
            float v = 0.f;
            if (o >= 0 && o < n) {
                const int t = o / a.n_coef, c = o - t * a.n_coef, x = t + kHalo;
                v = CARRIED && t + sh < a.T ? old[c * a.tp + x] : src[(size_t)c * a.ftp + x];
            }
            dst[i] = v;
        }
    } else {
        float* dst = a.windows + (size_t)b * a.n_coef * a.tp;
        const int n = a.n_coef * a.tp;
        const int dc = 256 / a.tp, dx = 256 - dc * a.tp;
        int c = threadIdx.x / a.tp, x = threadIdx.x - c * a.tp;
        for (int i = threadIdx.x; i < n; i += 256) {
            const int t = x - kHalo;
            dst[i] = t >= 0 && t < a.T ? (CARRIED && t + sh < a.T ? old[c * a.tp + x] : src[(size_t)c * a.ftp + x]) : 0.f;
            c += dc;
            x += dx;
            if (x >= a.tp) { x -= a.tp; ++c; }
        }
    }
}

// The state write-back, one workgroup per stream s = s0 + blockIdx.x of a range whose streams (RAGGED: those with steps; one without
// returns at once) all have their last group in the chunk.  Its last slot b, the call's length L for it and its samples: dense from
// groups / steps, RAGGED from the tables (the slots are compact: packed step step_off[s + 1] - 1 - p0; the stream's own packed samples).
// window = the last step's gathered window (planar, zero halo: the state's layout; PLANES: read back from the last step's plane,
// column t, coefficient c <- plane offset t n_coef + c); tail = the last tail_len samples of  tail ++ samples  (old samples that
// survive a short call are read into LDS before the tail is written).
template <bool PLANES, bool RAGGED>
__global__ __launch_bounds__(256) void scan_carry_kernel(const ScanChunkArgs a) {
    __shared__ float s_tail[kMaxTail];
    const int64_t s = a.s0 + blockIdx.x;
    const int tid = threadIdx.x;
    int64_t b, L;
    const float* src;
    if constexpr (RAGGED) {
        const int64_t first = a.step_off[s], m = a.step_off[s + 1] - first;
        if (m == 0) return;
        b = first + m - 1 - a.p0;
        L = m * a.k_hop;
        src = a.samples + first * a.k_hop;
    } else {
        b = (s * a.groups + a.groups - 1 - a.q0) * a.G + a.steps - 1 - (a.groups - 1) * a.G;
        L = a.L;
        src = a.samples + s * a.L;
    }
    const int win_elems = a.n_coef * a.tp;
    float* wdst = a.st.window + s * win_elems;
    if constexpr (PLANES) {
        const float* wsrc = a.windows + b * (a.T * a.n_coef + 2 * kHalo) + kHalo;
        for (int i = tid; i < win_elems; i += 256) {
            const int c = i / a.tp, t = i - c * a.tp - kHalo;
            wdst[i] = t >= 0 && t < a.T ? wsrc[t * a.n_coef + c] : 0.f;
        }
    } else {
        const float* wsrc = a.windows + b * win_elems;
        for (int i = tid; i < win_elems; i += 256) wdst[i] = wsrc[i];
    }
    const int tail_len = a.st.tail_len;
    const bool rst = scan_fresh(a.st, s);
    float* tail = a.st.tail + s * tail_len;
    const int keep = L < tail_len ? (int)(tail_len - L) : 0;                   // old tail samples L .. tail_len - 1 stay
    for (int i = tid; i < keep; i += 256) s_tail[i] = rst ? 0.f : tail[L + i];
    __syncthreads();
    for (int i = tid; i < tail_len; i += 256) tail[i] = i < keep ? s_tail[i] : src[L - tail_len + i];
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

struct ScanDetectArgs {
    const float* probs;         // [N][steps][C]
    float* smoothed;
    int32_t* top;               // [N][steps]
    float* score;
    int32_t* is_new;            // scan_smooth_kernel writes the candidate flag, top + 1 (candidate) or 0; scan_suppress_kernel the detections
    ScanState st;
    int64_t steps;
    int N, C, W, min_count, suppression;
    float threshold;
    const int64_t* step_off;    // ragged: [N + 1] (the rows are packed, `steps` is their total)
};

// A lane per (signal, step, class), 256 / C steps per workgroup: the streaming detector's smoothing over the last
// count = min(count0 + i + 1, W) probability vectors (smooth_mean, stream.hip: the same expression), those of steps before the call
// from ring slot (head0 + j) mod W (j < 0, oldest first); the argmax from LDS by the step's first lane, top / score (-1 / 0 below
// min_count) and the candidate flag.  Consecutive lanes read consecutive floats.  CARRIED: the call has a state; without one the
// ring is never read, and the instance has no test for it (at run time it doubled this kernel's time for tcr_scan).  RAGGED: w is
// a packed step; i is relative to its signal's first row, so count = min(i + 1, W) never reaches the previous signal's rows.
// CARRIED && RAGGED: the stream's own head0 and count0, the steps before the call from its ring slots.
// The kernel's body is scan_smooth, with one more compile-time axis, OUTS: what is written.  The scans' kernels are kSmoothAll and
// carry no test; kSmoothNoVector leaves `smoothed` out (tcr_detect_redetect with smoothed == NULL), kSmoothTopScore the candidate
// flag as well (tcr_detect_grid's per-pair path writes top / score rows only): detect_smooth_kernel, detect_grid.hip.
constexpr int kSmoothAll = 0, kSmoothNoVector = 1, kSmoothTopScore = 2;
template <bool CARRIED, bool RAGGED, int OUTS>
__device__ __forceinline__ void scan_smooth(const ScanDetectArgs& a) {
    __shared__ float s_sm[256];
    const int C = a.C, W = a.W;
    const int per = 256 / C;
    const int ls = threadIdx.x / C, c = threadIdx.x - ls * C;
    const int64_t w = (int64_t)blockIdx.x * per + ls;                   // window = s steps + i
    const bool live = ls < per && w < (RAGGED ? a.steps : a.N * a.steps);
    int count = 0;
    if (live) {
        int64_t s, i, row0;
        if constexpr (RAGGED) {
            s = ragged_signal(a.step_off, a.N, w);
            row0 = a.step_off[s];
            i = w - row0;
        } else {
            s = w / a.steps;
            i = w - s * a.steps;
            row0 = s * a.steps;
        }
        const bool fresh = !CARRIED || scan_fresh(a.st, s);
        const int head0 = fresh ? 0 : a.st.ist[s], count0 = fresh ? 0 : a.st.ist[a.N + s];
        count = count0 + i + 1 < W ? (int)(count0 + i + 1) : W;
        int64_t jj = i - count + 1;                                     // oldest step (< 0: before the call)
        int slot = jj < 0 ? (head0 + (int)jj < 0 ? head0 + (int)jj + W : head0 + (int)jj) : 0;
        const float* p = a.probs + row0 * C + c;
        const size_t ring_row = (size_t)a.N * C, sc = (size_t)s * C + c;
        const float v = smooth_mean(count, [&]() {
            float x;
            if (CARRIED && jj < 0) {
                x = a.st.ring[slot * ring_row + sc];
                slot = slot + 1 == W ? 0 : slot + 1;
            } else {
                x = p[jj * C];
            }
            ++jj;
            return x;
        });
        if constexpr (OUTS == kSmoothAll) a.smoothed[w * C + c] = v;
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
    if constexpr (OUTS != kSmoothTopScore) a.is_new[w] = warm && best_v > a.threshold ? best + 1 : 0;
}

template <bool CARRIED, bool RAGGED = false>
__global__ __launch_bounds__(256) void scan_smooth_kernel(const ScanDetectArgs a) {
    scan_smooth<CARRIED, RAGGED, kSmoothAll>(a);
}

// One workgroup per signal: the ring write-back, the suppression walk from the carried detector, the detector integers.  The walk goes
// over the signal's flags in passes of 256 x kSuppressPer, read coalesced into LDS.  A pass without a candidate costs its loads and
// two barriers.  Otherwise wave 0 looks for the next detection: fired = top != prev_label && (prev_label == -1 || i - prev_step >
// suppression), so after a detection the walk jumps past the suppressed steps, and from there the first candidate whose label differs
// from prev_label fires -- 256 steps per probe (four per lane, the lowest index by a butterfly minimum), one probe per detection or
// per 256 steps.  A detection is marked -1 in LDS; then the candidates' flags are rewritten as 0 / 1.  Non-candidates never fire and
// never change the state.  RAGGED: the signal's rows start at step_off[s] and there are step_off[s + 1] - step_off[s] of them; a signal
// without steps returns at once.
template <bool RAGGED>
__global__ __launch_bounds__(256) void scan_suppress_kernel(const ScanDetectArgs a) {
    constexpr int PASS = 256 * kSuppressPer;
    constexpr int NONE = 0x7fffffff;
    __shared__ int s_val[PASS];
    __shared__ int s_any[2];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, C = a.C, W = a.W;
    const int64_t row0 = RAGGED ? a.step_off[s] : (int64_t)s * a.steps;
    const int64_t steps = RAGGED ? a.step_off[s + 1] - row0 : a.steps;
    if (RAGGED && steps == 0) return;
    int* ist = a.st.ist;
    const bool fresh = scan_fresh(a.st, s);
    const int head0 = fresh ? 0 : ist[s], count0 = fresh ? 0 : ist[N + s];
    const int n0 = fresh ? 0 : ist[4 * N + s];
    int prev_label = fresh ? -1 : ist[2 * N + s];                       // (wave 0's, the same in its lanes)
    int64_t prev_step = fresh ? 0 : (int64_t)ist[3 * N + s] - n0;       // relative to the call's first step: may be negative
    if (a.st.ring) {
        const int nw = steps < W ? (int)steps : W;                      // the last nw vectors stay in the ring
        const int64_t i0 = steps - nw;
        for (int e = tid; e < nw * C; e += 256) {
            const int d = e / C, c = e - d * C;
            const int slot = (int)((head0 + i0 + d) % W);
            a.st.ring[(size_t)slot * N * C + (size_t)s * C + c] = a.probs[(row0 + i0 + d) * C + c];
        }
    }
    int32_t* fl = a.is_new + row0;
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
                    const int64_t lo = prev_step + a.suppression + 1 - base;
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
    if (ist && tid == 0) {                                              // (every thread read the integers before the walk's barriers)
        ist[s] = (int)((head0 + steps) % W);
        ist[N + s] = count0 + steps < W ? (int)(count0 + steps) : W;
        ist[2 * N + s] = prev_label;
        ist[3 * N + s] = (int)(n0 + prev_step);
        ist[4 * N + s] = (int)(n0 + steps);
    }
}

namespace {

// scan_suppress_kernel over da's signals: the last launch of every detector tail
int suppress_launch(const ScanDetectArgs& da, bool ragged, hipStream_t s) {
    const auto suppress = ragged ? scan_suppress_kernel<true> : scan_suppress_kernel<false>;
    hipLaunchKernelGGL(suppress, dim3(da.N), dim3(256), 0, s, da);
    return check_launch("scan_suppress_kernel");
}

// what the entries over a scan's rows refuse about their number: n signals or streams (`whose`), steps (dense) / total_steps (ragged) ...
int detect_rows_check(const char* what, bool ragged, int n, int64_t steps, int64_t total_steps, const char* whose) {
    TCR_REQUIRE(n > 0, "%s: the number of %s must be positive (got %d)", what, whose, n);
    TCR_REQUIRE(ragged ? total_steps > 0 : steps > 0, "%s: the number of steps must be positive (got %lld)", what,
                (long long)(ragged ? total_steps : steps));
    return TCR_OK;
}

// ... and about their size, at the wider of the input and output rows' columns
int detect_size_check(const char* what, bool ragged, int n, int64_t steps, int64_t total_steps, int in_cols, int out_cols) {
    const int64_t rows = ragged ? total_steps : steps * n;
    const int widest = in_cols > out_cols ? in_cols : out_cols;
    TCR_REQUIRE((ragged || steps < ((int64_t)1 << 31)) && rows < ((int64_t)1 << 31) && rows * widest < ((int64_t)1 << 31),
                "%s: %lld steps in all x %d columns is too large", what, (long long)rows, widest);
    return TCR_OK;
}

struct ScanOutputs {
    float *logits, *probs, *smoothed;   // [N][steps][C] (ragged: [total_steps][C])
    int32_t* top;                       // [N][steps]
    float* score;
    int32_t* is_new;
};

// One call of the four entries, as the extern "C" functions fill it; scan_entry checks it and completes io, tables and the workspace.
struct ScanCall {
    const tcr_frontend_cfg* cfg;
    const void* plan_dev;
    const tcr_model_ref* m;
    ModelIO io;
    int n, k;                           // signals (streams), frames per step
    const tcr_detect_cfg* det;
    const float* samples;
    const uint8_t* reset;               // [n] or null
    void* state;                        // the stream state (stream.hip); read only when `carried`
    bool carried;                       // the call starts from `state` and writes it back: the n signals are its streams
    void* workspace;
    size_t ws_bytes;
    int64_t* tables;                    // ragged: the device tables [2][n + 1] (step offsets, then group offsets), the workspace's front
    ScanOutputs out;
    void* stream;
    const char* what;
};

// the front-end row length for `steps` steps: at most kScanGroup (and max_windows) steps, balanced so the groups of a signal differ
// by at most one step from each other in size
int scan_group(int64_t steps, int cap) {
    const int64_t g0 = std::min<int64_t>(std::min(kScanGroup, cap), steps);
    const int64_t groups = ceil_div64(steps, g0);
    return (int)ceil_div64(steps, groups);
}

size_t scan_ragged_tables_bytes(int64_t n_signals) { return (size_t)round_up64(2 * (n_signals + 1) * (int64_t)sizeof(int64_t), 256); }

// Front-end rows of a ragged call at group size G (every group is a row of G k + T - k frames, whatever its live steps)
int64_t scan_ragged_groups(const int64_t* so, int n_signals, int G) {
    int64_t rows = 0;
    for (int n = 0; n < n_signals; ++n) rows += ceil_div64(so[n + 1] - so[n], G);
    return rows;
}

// The largest chunk the workspace holds: G by the call's policy, then R rows (TCR_ERR_WORKSPACE below one window).  R G also stays
// within io.max_batch (scan_geom_ok; G <= kScanGroup is far below every family's bound), so that every window of a DS-CNN scan runs on
// the kernel path a stream step of up to kDscnnMaxBatch streams runs.  The results do not depend on the chunking, so G is a cost
// choice only.  Dense (so == null, n x steps): the balanced group, smaller when even one row of it does not fit.  Ragged (so: the
// step offsets [n + 1]): G, at most kScanGroup, the longest signal and what one row of the workspace holds, with the fewest front-end
// frames over the call (ties: the larger G, fewer rows); the sum is evaluated for every candidate while n x candidates stays small,
// for every few otherwise.
int scan_chunking(const ScanCall& c, int64_t steps, const int64_t* so, ScanGeom& out) {
    const int k = c.k, T = c.cfg->n_frames;
    const auto bytes = [&](int G, int64_t R) { return (size_t)scan_geom(*c.cfg, *c.m, c.io, k, G, (int)R).ws_floats * sizeof(float); };
    const auto fits = [&](int G, int64_t R) { return scan_geom_ok(k, T, G, R, c.io.max_batch) && bytes(G, R) <= c.ws_bytes; };
    // the largest v of lo .. hi with ok(v), lo when there is none (binary search; the size grows with R and with G)
    const auto largest = [](int64_t lo, int64_t hi, const auto& ok) {
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (ok(mid)) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    };
    if (!fits(1, 1)) {
        set_error("%s: workspace %zu bytes < one window's %zu", c.what, c.ws_bytes, bytes(1, 1));
        return TCR_ERR_WORKSPACE;
    }
    int G;
    int64_t total_groups;
    if (!so) {
        G = scan_group(steps, kScanGroup);
        while (G > 1 && bytes(G, 1) > c.ws_bytes) G = scan_group(steps, G / 2);
        total_groups = ceil_div64(steps, G) * c.n;
    } else {
        int64_t longest = 1;
        for (int n = 0; n < c.n; ++n) longest = std::max(longest, so[n + 1] - so[n]);
        const int g_max = (int)largest(1, std::min<int64_t>(kScanGroup, longest), [&](int64_t g) { return fits((int)g, 1); });
        const auto frames = [&](int g) { return scan_ragged_groups(so, c.n, g) * ((int64_t)g * k + T - k); };
        const int stride = (int)std::max<int64_t>(1, ceil_div64((int64_t)c.n * g_max, (int64_t)1 << 22));
        G = g_max;
        int64_t best = frames(G);
        for (int g = g_max - stride; g >= 1; g -= stride) {
            const int64_t f = frames(g);
            if (f < best) { best = f; G = g; }
        }
        total_groups = scan_ragged_groups(so, c.n, G);
    }
    out = scan_geom(*c.cfg, *c.m, c.io, k, G, (int)largest(1, total_groups, [&](int64_t R) { return fits(G, R); }));
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

// The pipeline of the header comment over a checked call: n x steps (dense, so empty) or the step offsets so [n + 1] (ragged), from
// and to the state st (all null: none).  The dense and the ragged form differ at the five places marked (1) .. (5).
int scan_run(const ScanCall& c, const ScanState& st, int64_t steps, const std::vector<int64_t>& so) {
    const tcr_frontend_cfg& cfg = *c.cfg;
    const bool ragged = !so.empty(), carried = st.window != nullptr;
    const int N = c.n, k = c.k;
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    ScanGeom g;
    TCR_TRY(scan_chunking(c, steps, ragged ? so.data() : nullptr, g));
    const int G = g.G;
    float* ws = static_cast<float*>(c.workspace);
    ScanChunkArgs ca{};
    ca.samples = c.samples; ca.stage = ws + g.stage_off; ca.frames = ws + g.frames_off; ca.windows = ws + g.win_off; ca.st = st;
    ca.k_hop = (int64_t)k * cfg.hop; ca.stride = g.stage_stride; ca.n_prefix = cfg.n_samples; ca.G = G; ca.k = k; ca.T = g.T; ca.tp = g.tp;
    ca.n_coef = g.n_coef; ca.ftp = tcr_padded_len(g.F);
    // the flattened groups: dense, `groups` per signal; ragged, the table go [N + 1] next to so, both uploaded
    std::vector<int64_t> tables;
    const int64_t* go = nullptr;
    int64_t groups = 0, total_groups, total_steps;
    if (ragged) {
        tables.resize(2 * ((size_t)N + 1));
        std::copy(so.begin(), so.end(), tables.begin());
        int64_t* t = tables.data() + N + 1;
        t[0] = 0;
        for (int n = 0; n < N; ++n) t[n + 1] = t[n] + ceil_div64(so[n + 1] - so[n], G);
        go = t;
        total_groups = go[N]; total_steps = so[N];
        // the tables live on the host's stack frame: the copy is complete before the call returns (and before the first launch)
        if (hipMemcpyAsync(c.tables, tables.data(), tables.size() * sizeof(int64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess) {
            set_error("%s: the upload of the offset tables failed", c.what);
            return TCR_ERR_HIP;
        }
        ca.step_off = c.tables; ca.group_off = c.tables + N + 1; ca.n_sig = N;
    } else {
        groups = ceil_div64(steps, G);
        total_groups = groups * N; total_steps = N * steps;
        ca.L = steps * ca.k_hop; ca.groups = groups; ca.steps = steps;
    }
    // ragged: the packed step of flattened group q's first slot
    const auto first_step = [&](int64_t q) {
        if (q >= total_groups) return total_steps;
        const int64_t n = std::upper_bound(go, go + N + 1, q) - go - 1;
        return so[n] + (q - go[n]) * G;
    };
    const auto stage_ragged = carried ? scan_stage_ragged_kernel<true> : scan_stage_ragged_kernel<false>;
    const auto gather = g.planes ? (carried ? (ragged ? scan_gather_kernel<true, true, true> : scan_gather_kernel<true, true, false>)
                                            : (ragged ? scan_gather_kernel<true, false, true> : scan_gather_kernel<true, false, false>))
                                 : (carried ? (ragged ? scan_gather_kernel<false, true, true> : scan_gather_kernel<false, true, false>)
                                            : (ragged ? scan_gather_kernel<false, false, true> : scan_gather_kernel<false, false, false>));
    const auto carry = g.planes ? (ragged ? scan_carry_kernel<true, true> : scan_carry_kernel<true, false>)
                                : (ragged ? scan_carry_kernel<false, true> : scan_carry_kernel<false, false>);
    const int64_t stage_blocks = ceil_div64(g.stage_stride, 256);
    int next = 0;                                       // ragged, carried: the first stream whose write-back is still to come
    for (int64_t q0 = 0; q0 < total_groups; q0 += g.R) {
        const int rows = (int)std::min<int64_t>(g.R, total_groups - q0);
        ca.q0 = q0; ca.rows = rows;
        // (1) the staging launch
        if (ragged) {
            const int bx = (int)std::max<int64_t>(1, std::min(stage_blocks, ceil_div64(8 * (int64_t)device_cus(), rows)));
            hipLaunchKernelGGL(stage_ragged, dim3((unsigned)((int64_t)rows * bx)), dim3(256), 0, s, ca, bx);
        } else {
            const int64_t staged = (int64_t)rows * g.stage_stride;
            hipLaunchKernelGGL(scan_stage_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(staged, 256), 8 * (int64_t)device_cus())), dim3(256), 0,
                               s, ca);
        }
        TCR_TRY(check_launch(ragged ? "scan_stage_ragged_kernel" : "scan_stage_kernel"));
        TCR_TRY(stream_frontend(cfg, c.plan_dev, ca.stage, g.stage_stride, rows, g.F, ca.frames, s, ca.ftp));
        // (2) the slots: every step of the rows, or (a signal's groups cover its steps in order) the live steps p0 .. p(q0 + rows) - 1
        int slots = rows * G;
        if (ragged) {
            ca.p0 = first_step(q0);
            slots = (int)(first_step(q0 + rows) - ca.p0);
        }
        hipLaunchKernelGGL(gather, dim3(slots), dim3(256), 0, s, ca);
        TCR_TRY(check_launch("scan_gather_kernel"));
        // (3) the write-back range: the streams whose last group is one of this chunk's rows.  Dense: group s groups + groups - 1.
        // Ragged: go[n + 1] - 1, increasing over the streams with steps; next .. the last such one, streams without steps in between
        // included (their workgroups return at once)
        if (carried) {
            int64_t s_lo = N, s_hi = -1;
            if (ragged) {
                for (; next < N && (so[next + 1] == so[next] || go[next + 1] - 1 < q0 + rows); ++next) {
                    if (so[next + 1] == so[next]) continue;
                    s_lo = std::min<int64_t>(s_lo, next);
                    s_hi = next;
                }
            } else {
                s_lo = (q0 + 1 + groups - 1) / groups - 1;
                s_hi = (q0 + rows) / groups - 1;
            }
            if (s_hi >= s_lo) {
                ca.s0 = s_lo;
                hipLaunchKernelGGL(carry, dim3((unsigned)(s_hi - s_lo + 1)), dim3(256), 0, s, ca);
                TCR_TRY(check_launch("scan_carry_kernel"));
            }
        }
        // (4) the network's outputs: the chunk's slots in the workspace, or the live steps' rows of the caller's
        float* logits = ragged ? c.out.logits + ca.p0 * g.classes : ws + g.logits_off;
        float* probs = ragged ? c.out.probs + ca.p0 * g.classes : ws + g.probs_off;
        TCR_TRY(model_forward(*c.m, ca.windows, slots, ws + g.net_off, c.ws_bytes - (size_t)g.net_off * sizeof(float), logits, probs, c.stream));
        // (5) the scatter of the slots that are steps
        if (!ragged) {
            ScanScatterArgs xa;
            xa.logits_in = logits; xa.probs_in = probs; xa.logits = c.out.logits; xa.probs = c.out.probs; xa.q0 = q0;
            xa.groups = groups; xa.steps = steps; xa.G = G; xa.C = g.classes; xa.slots = slots;
            hipLaunchKernelGGL(scan_scatter_kernel, dim3(ceil_div(slots * g.classes, 256)), dim3(256), 0, s, xa);
            TCR_TRY(check_launch("scan_scatter_kernel"));
        }
    }
    // the detector tail, once per call
    ScanDetectArgs da;
    da.probs = c.out.probs; da.smoothed = c.out.smoothed; da.top = c.out.top; da.score = c.out.score; da.is_new = c.out.is_new; da.st = st;
    da.steps = ragged ? total_steps : steps; da.N = N; da.C = g.classes; da.W = c.det->average_steps; da.min_count = c.det->min_count;
    da.suppression = c.det->suppression_steps; da.threshold = c.det->threshold; da.step_off = ragged ? c.tables : nullptr;
    const auto smooth = carried ? (ragged ? scan_smooth_kernel<true, true> : scan_smooth_kernel<true, false>)
                                : (ragged ? scan_smooth_kernel<false, true> : scan_smooth_kernel<false, false>);
    hipLaunchKernelGGL(smooth, dim3((unsigned)ceil_div64(total_steps, 256 / g.classes)), dim3(256), 0, s, da);
    TCR_TRY(check_launch("scan_smooth_kernel"));
    return suppress_launch(da, ragged, s);
}

// The step offsets so [n + 1] of a ragged call's sample_offsets (HOST [n + 1]), with every refusal about them.
int scan_step_offsets(const char* what, const char* noun, int n_signals, int64_t khop, int classes, const int64_t* sample_offsets,
                      std::vector<int64_t>& so) {
    TCR_REQUIRE(sample_offsets[0] == 0, "%s: sample_offsets must start at 0 (got %lld)", what, (long long)sample_offsets[0]);
    so.resize((size_t)n_signals + 1);
    so[0] = 0;
    for (int n = 0; n < n_signals; ++n) {
        const int64_t len = sample_offsets[n + 1] - sample_offsets[n];
        TCR_REQUIRE(len >= 0, "%s: sample_offsets decrease at %s %d (%lld after %lld)", what, noun, n, (long long)sample_offsets[n + 1],
                    (long long)sample_offsets[n]);
        TCR_REQUIRE(len % khop == 0, "%s: the length %lld of %s %d is not a multiple of k * hop = %lld", what, (long long)len, noun, n,
                    (long long)khop);
        so[n + 1] = so[n] + len / khop;
    }
    TCR_REQUIRE(so[n_signals] > 0, "%s: no %s has a whole step (total_steps == 0)", what, noun);
    TCR_REQUIRE(so[n_signals] * classes < ((int64_t)1 << 31), "%s: %lld steps in all is too large", what, (long long)so[n_signals]);
    return TCR_OK;
}

// The checks of the four entries, in one order; then the state's regions and the pipeline.  Dense (sample_offsets == null): n_samples
// per signal become `steps`.  Ragged: sample_offsets [n + 1] become step offsets, the tables take the workspace's front, and samples
// and outputs may be null up to the late check (a caller sizes its outputs by what the offsets yield).  With a state the n signals are
// its streams (a stream without steps is allowed, a call without any step is not), and the messages say so.
int scan_entry(ScanCall& c, bool ragged, int64_t n_samples, const int64_t* sample_offsets) {
    const char* what = c.what;
    const char* noun = c.carried ? "stream" : "signal";
    const ScanOutputs& o = c.out;
    const bool io_ptrs = c.samples && o.logits && o.probs && o.smoothed && o.top && o.score && o.is_new;
    TCR_REQUIRE(c.plan_dev && c.m && c.m->params && c.m->aux && c.det && c.workspace && (!c.carried || c.state) &&
                (ragged ? sample_offsets != nullptr : io_ptrs), "%s: null argument", what);
    if (!c.carried) TCR_REQUIRE(c.n > 0, "%s: the number of signals must be positive (got %d)", what, c.n);
    TCR_TRY(stream_check(c.cfg, c.m, c.n, c.k, c.det, what, c.io, c.carried));
    const int64_t khop = (int64_t)c.k * c.cfg->hop;
    int64_t steps = 0;
    std::vector<int64_t> so;
    if (!ragged) {
        TCR_REQUIRE(n_samples > 0 && n_samples % khop == 0, "%s: the signal length %lld is not a positive multiple of k * hop = %lld", what,
                    (long long)n_samples, (long long)khop);
        steps = n_samples / khop;
        TCR_REQUIRE((int64_t)c.n * steps * c.io.classes < ((int64_t)1 << 31), "%s: %d %ss x %lld steps is too large", what, c.n, noun,
                    (long long)steps);
    } else {
        const size_t tables_bytes = scan_ragged_tables_bytes(c.n);
        TCR_REQUIRE(tables_bytes <= c.ws_bytes, "%s: %d %ss are more than the max_signals the workspace's offset tables hold (%lld)", what,
                    c.n, noun, (long long)(c.ws_bytes / (2 * sizeof(int64_t))) - 1);
        TCR_TRY(scan_step_offsets(what, noun, c.n, khop, c.io.classes, sample_offsets, so));
        TCR_REQUIRE(io_ptrs, "%s: null argument", what);
        c.tables = static_cast<int64_t*>(c.workspace);
        c.workspace = static_cast<char*>(c.workspace) + tables_bytes;
        c.ws_bytes -= tables_bytes;
    }
    ScanState st{};
    if (c.carried) {
        const StreamGeom sg = stream_geom(*c.cfg, *c.m, c.io, c.n, c.k, c.det->average_steps);
        float* f = static_cast<float*>(c.state);
        st = ScanState{f + sg.win_off, f + sg.tail_off, f + sg.ring_off, reinterpret_cast<int*>(f + sg.ist_off), c.reset, sg.tail_len};
    }
    return scan_run(c, st, steps, so);
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

extern "C" size_t tcr_scan_ragged_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int k, int max_windows,
                                                  int max_signals) {
    const size_t chunk = scan_workspace_bytes(cfg, model, k, max_windows, "tcr_scan_ragged_workspace_bytes");
    if (chunk == 0) return 0;
    if (max_signals < 1) { set_error("tcr_scan_ragged_workspace_bytes: max_signals must be >= 1 (got %d)", max_signals); return 0; }
    return scan_ragged_tables_bytes(max_signals) + chunk;
}

extern "C" int tcr_scan_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_signals, int64_t n_samples,
                          int k, const tcr_detect_cfg* det, const float* samples, void* workspace, size_t ws_bytes, float* logits,
                          float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    ScanCall c{cfg, plan_dev, model, {}, n_signals, k, det, samples, nullptr, nullptr, false, workspace, ws_bytes, nullptr,
               {logits, probs, smoothed, top, score, is_new}, stream, "tcr_scan_m"};
    return scan_entry(c, false, n_samples, nullptr);
}

extern "C" int tcr_scan(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params, const float* frozen_ss,
                        int n_signals, int64_t n_samples, int k, const tcr_detect_cfg* det, const float* samples, void* workspace,
                        size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                        void* stream) {
    const tcr_model_ref m = tcresnet_ref(net, params, frozen_ss);
    ScanCall c{cfg, plan_dev, &m, {}, n_signals, k, det, samples, nullptr, nullptr, false, workspace, ws_bytes, nullptr,
               {logits, probs, smoothed, top, score, is_new}, stream, "tcr_scan"};
    return scan_entry(c, false, n_samples, nullptr);
}

extern "C" int tcr_stream_scan_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams,
                                 int64_t n_samples, int k, const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state,
                                 void* workspace, size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score,
                                 int32_t* is_new, void* stream) {
    ScanCall c{cfg, plan_dev, model, {}, n_streams, k, det, samples, reset, state, true, workspace, ws_bytes, nullptr,
               {logits, probs, smoothed, top, score, is_new}, stream, "tcr_stream_scan_m"};
    return scan_entry(c, false, n_samples, nullptr);
}

extern "C" int tcr_stream_scan(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                               const float* frozen_ss, int n_streams, int64_t n_samples, int k, const tcr_detect_cfg* det,
                               const float* samples, const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, float* logits,
                               float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    const tcr_model_ref m = tcresnet_ref(net, params, frozen_ss);
    ScanCall c{cfg, plan_dev, &m, {}, n_streams, k, det, samples, reset, state, true, workspace, ws_bytes, nullptr,
               {logits, probs, smoothed, top, score, is_new}, stream, "tcr_stream_scan"};
    return scan_entry(c, false, n_samples, nullptr);
}

extern "C" int tcr_scan_ragged(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_signals,
                               const int64_t* sample_offsets, int k, const tcr_detect_cfg* det, const float* samples, void* workspace,
                               size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                               void* stream) {
    ScanCall c{cfg, plan_dev, model, {}, n_signals, k, det, samples, nullptr, nullptr, false, workspace, ws_bytes, nullptr,
               {logits, probs, smoothed, top, score, is_new}, stream, "tcr_scan_ragged"};
    return scan_entry(c, true, 0, sample_offsets);
}

extern "C" int tcr_stream_scan_ragged_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams,
                                        const int64_t* sample_offsets, int k, const tcr_detect_cfg* det, const float* samples,
                                        const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, float* logits, float* probs,
                                        float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    ScanCall c{cfg, plan_dev, model, {}, n_streams, k, det, samples, reset, state, true, workspace, ws_bytes, nullptr,
               {logits, probs, smoothed, top, score, is_new}, stream, "tcr_stream_scan_ragged_m"};
    return scan_entry(c, true, 0, sample_offsets);
}

extern "C" int tcr_stream_scan_ragged(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                                      const float* frozen_ss, int n_streams, const int64_t* sample_offsets, int k, const tcr_detect_cfg* det,
                                      const float* samples, const uint8_t* reset, void* state, void* workspace, size_t ws_bytes,
                                      float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                                      void* stream) {
    const tcr_model_ref m = tcresnet_ref(net, params, frozen_ss);
    ScanCall c{cfg, plan_dev, &m, {}, n_streams, k, det, samples, reset, state, true, workspace, ws_bytes, nullptr,
               {logits, probs, smoothed, top, score, is_new}, stream, "tcr_stream_scan_ragged"};
    return scan_entry(c, true, 0, sample_offsets);
}
