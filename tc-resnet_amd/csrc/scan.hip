// Many detector steps in one call: tcr_stream_scan advances S streams by m steps from their stream state (stream.hip) and writes the
// state back, bitwise m calls of tcr_stream_step -- outputs and state; tcr_scan is the same call from a fresh state without the
// write-back: every step of N recordings, bitwise what a fresh streaming detector returns push by push.  One pipeline runs both; the
// state (ScanState) is its variable part, and "fresh" is what reset[s] != 0 means as well.
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
// Steps are cut into groups of G consecutive steps of one signal; group g of signal n is one front-end row of F = G k + T - k frames
// from new frame g G k + k - T on.  A chunk is R consecutive groups (flattened over signals) = R G window slots:
//   scan_stage_kernel     the R staging rows (tail ++ samples, zeros outside);
//   frontend_pk3_kernel   <.., STREAM = true> over R rows of F frames into frame rows [R][n_coef][F + 2 TCR_HALO] (column 0 on);
//   scan_gather_kernel    the windows from the frame rows, or from carried columns for negative frames: planar
//                         [R G][n_coef][T + 2 TCR_HALO] (zero halo), or the 2-D graph's planes [R G][1][T n_coef + 2 TCR_HALO];
//   scan_carry_kernel     with a state: window and tail write-back of the streams whose last group is in this chunk (their last
//                         step's window, gathered just before; the last tail_len samples of x, the old tail read before it is
//                         written); a stream's groups are consecutive, so no later chunk reads its window or tail;
//   the network at batch R G (detect_model.h: tcr_net_forward_frozen, tcr_dscnn_forward_infer or tcr_g2d_forward_infer, unchanged);
//   scan_scatter_kernel   logits / probs of the slots that are steps (g G + j < steps) into the caller's [N][steps][C].
// Slots past a signal's last step (the last group of a signal may be short) are computed and dropped.  Then, once per call:
//   scan_smooth_kernel    a lane per (signal, step, class): smoothed over count_i = min(count0 + i + 1, W) vectors, those of steps
//                         before the call from ring slots (head0 - d) mod W, oldest first; top, score and the candidate flag
//                         (is_new = top + 1 or 0);
//   scan_suppress_kernel  a workgroup per signal: the ring write-back (the last min(W, m) vectors at slots (head0 + i) mod W: the
//                         smoothing has read the old ones), the detections in step order from the carried prev_label and
//                         prev_step - n0, rewritten into is_new, then the five detector integers.
//
// Ragged (tcr_scan_ragged): N fresh signals of different lengths, packed.  The same stages, with two prefix tables in place of
// q / groups and n steps + i: step_off [N + 1] (signal n's steps are packed rows step_off[n] ..) and, once G is chosen, group_off
// [N + 1] (its ceil(steps_n / G) groups are flattened rows group_off[n] ..); the host builds both and uploads them to the front of
// the workspace, and the kernels find the signal of a flattened group or a packed step by binary search (ragged_signal).  A signal's
// groups cover its steps in order, so a chunk's live steps are one contiguous range of packed steps: the gather writes them
// compactly (slot = p - p(q0)), the network runs at the batch of the live steps and writes their rows of the caller's logits /
// probs itself -- no scatter, and the dead slots of a short last group cost front-end frames only.  The smoothing counts from the
// signal's first row and the suppression walks the signal's own rows, so a signal's rows are bitwise its dense scan alone.  G is
// the group size with the fewest front-end frames over the call (scan_ragged_chunking).  The ragged arms are compile-time instances
// (RAGGED) or sibling kernels: the dense instances carry no test for them.
//
// Ragged with a state (tcr_stream_scan_ragged): stream s advances by m_s >= 0 steps of its own, samples and rows packed as above.  The
// ragged stages with the carried arms: the staging row reads the stream's tail in front of its samples (scan_stage_ragged_tail_kernel;
// with a small G several groups of a stream reach into the prefix), the gather takes the first T - (i + 1) k columns of a stream's
// early steps from its carried window (CARRIED && RAGGED), the smoothing counts from the stream's count0 and reads its ring, the
// suppression is the ragged instance run with the state, and scan_carry_ragged_kernel writes window and tail back.  State ordering:
// the flattened groups are ordered by stream (group_off), so a stream's groups are consecutive rows here too and the dense argument
// holds -- a stream's window and tail are written only in the chunk that holds its last group, group_off[s + 1] - 1, after that
// chunk's stage and gather, and no later chunk has a group of that stream; ring and integers are written by the suppression, after
// the smoothing of every stream has read them.  A stream without steps (m_s == 0) has no group, no row and no carry, and its
// suppression workgroup returns before it reads or writes anything: its window, tail, ring and five integers are byte for byte what
// they were -- and so reset[s] != 0 with m_s == 0 is ignored (the caller keeps it for the call that brings the stream's next step).
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
    int tail_len;
};

__device__ __forceinline__ bool scan_fresh(const ScanState& st, int64_t s) { return !st.window || (st.reset && st.reset[s]); }

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
// zeros  (n_prefix = the clip's n_samples = T hop + tail_len), with the stream's tail in the last tail_len samples of the prefix.
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
// Signal n's samples start at step_off[n] k hop of the packed buffer and it is fresh: zeros in front and behind.
__global__ __launch_bounds__(256) void scan_stage_ragged_kernel(const ScanChunkArgs a, const int bx) {
    const int64_t r = blockIdx.x / (unsigned)bx;
    const int part = (int)(blockIdx.x - (unsigned)r * bx);
    const int64_t q = a.q0 + r;
    const int n = ragged_signal(a.group_off, a.n_sig, q);
    const int64_t g = q - a.group_off[n];
    const int64_t first = a.step_off[n], len = (a.step_off[n + 1] - first) * a.k_hop;
    const float* src = a.samples + first * a.k_hop;
    const int64_t base = (g * a.G + 1) * a.k_hop - a.n_prefix;
    float* dst = a.stage + r * a.stride;
    for (int64_t x = (int64_t)part * 256 + threadIdx.x; x < a.stride; x += (int64_t)bx * 256) {
        const int64_t pos = base + x;
        dst[x] = pos >= 0 && pos < len ? src[pos] : 0.f;
    }
}

// The ragged staging row of a call with a state: positions before the call come from the last tail_len samples of the prefix, the
// stream's tail (zeros when it is fresh); everything else is scan_stage_ragged_kernel.
__global__ __launch_bounds__(256) void scan_stage_ragged_tail_kernel(const ScanChunkArgs a, const int bx) {
    const int64_t r = blockIdx.x / (unsigned)bx;
    const int part = (int)(blockIdx.x - (unsigned)r * bx);
    const int64_t q = a.q0 + r;
    const int n = ragged_signal(a.group_off, a.n_sig, q);
    const int64_t g = q - a.group_off[n];
    const int64_t first = a.step_off[n], len = (a.step_off[n + 1] - first) * a.k_hop;
    const float* src = a.samples + first * a.k_hop;
    const int tail_len = a.st.tail_len;
    const float* tail = scan_fresh(a.st, n) ? nullptr : a.st.tail + (size_t)n * tail_len + tail_len;      // (indexed by pos < 0)
    const int64_t base = (g * a.G + 1) * a.k_hop - a.n_prefix;
    float* dst = a.stage + r * a.stride;
    for (int64_t x = (int64_t)part * 256 + threadIdx.x; x < a.stride; x += (int64_t)bx * 256) {
        const int64_t pos = base + x;
        float v = 0.f;
        if (pos >= 0) {
            if (pos < len) v = src[pos];
        } else if (tail && pos + tail_len >= 0) {
            v = tail[pos];
        }
        dst[x] = v;
    }
}

// One workgroup per window slot b = r G + j (step i = g G + j): column t is column j k + t of frame row r when new frame
// (i + 1) k - T + t >= 0 or the signal is fresh, else column (i + 1) k + t of the carried window; the halo is zero.  PLANES (2-D
// graph): the same window as its [T x n_coef] plane, written in plane order (coalesced): plane offset t n_coef + c <- window column t,
// coefficient c (features_to_plane_kernel's map, net2d_kernels.hip).  A pure copy: bitwise the planar gather followed by
// features_to_plane_kernel.  CARRIED: the call has a state; without one no column is carried, and the instance is the plain copy
// (the test at run time cost tcr_scan 5 % of this kernel, profiles/scan_unify_kernel_stats.csv).  RAGGED: the windows are compact --
// slot b is packed step p0 + b, whose signal, step, group and frame row come from the prefix tables -- so the chunk's slots are
// its live steps only and the network writes their rows of the caller's outputs itself.  CARRIED && RAGGED: the slot's signal is a
// stream of the state and i its step within the call, so the carried columns are those of the dense arm.
template <bool PLANES, bool CARRIED, bool RAGGED = false>
__global__ __launch_bounds__(256) void scan_gather_kernel(const ScanChunkArgs a) {
    const int b = blockIdx.x;
    int r, j;
    int64_t rs = 0, ri1 = 0;                                                    // RAGGED: the slot's stream and (i + 1) k
    if constexpr (RAGGED) {
        const int64_t p = a.p0 + b;
        const int n = ragged_signal(a.step_off, a.n_sig, p);
        const int64_t i = p - a.step_off[n], g = i / a.G;
        j = (int)(i - g * a.G);
        r = (int)(a.group_off[n] + g - a.q0);
        rs = n;
        ri1 = (i + 1) * a.k;
    } else {
        r = b / a.G;
        j = b - r * a.G;
    }
    const float* src = a.frames + (size_t)r * a.n_coef * a.ftp + j * a.k;      // window column x <- frame-row column j k + x
    const float* old = src;                                                     // (not read while sh = T)
    int sh = a.T;                                                               // carried columns: t < T - sh
    if constexpr (CARRIED && RAGGED) {
        if (ri1 < a.T && !scan_fresh(a.st, rs)) sh = (int)ri1;
        old = a.st.window + (size_t)rs * a.n_coef * a.tp + sh;
    } else if constexpr (CARRIED) {
        const int64_t q = a.q0 + r, s = q / a.groups, g = q - s * a.groups;
        const int64_t i1 = (g * a.G + j + 1) * a.k;                             // (i + 1) k
        if (i1 < a.T && !scan_fresh(a.st, s)) sh = (int)i1;
        old = a.st.window + (size_t)s * a.n_coef * a.tp + sh;
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

// One workgroup per stream s0 + blockIdx.x whose last group is in the chunk: window = its last step's gathered window (planar, zero
// halo: the state's layout; PLANES: read back from the last step's plane, column t, coefficient c <- plane offset t n_coef + c);
// tail = the last tail_len samples of  tail ++ samples  (old samples that survive a short call are read into LDS before the tail is
// written).
template <bool PLANES>
__global__ __launch_bounds__(256) void scan_carry_kernel(const ScanChunkArgs a) {
    __shared__ float s_tail[kMaxTail];
    const int64_t s = a.s0 + blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t b = (s * a.groups + a.groups - 1 - a.q0) * a.G + a.steps - 1 - (a.groups - 1) * a.G;
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
    const float* src = a.samples + s * a.L;
    const int keep = a.L < tail_len ? (int)(tail_len - a.L) : 0;               // old tail samples L .. tail_len - 1 stay
    for (int i = tid; i < keep; i += 256) s_tail[i] = rst ? 0.f : tail[a.L + i];
    __syncthreads();
    for (int i = tid; i < tail_len; i += 256) tail[i] = i < keep ? s_tail[i] : src[a.L - tail_len + i];
}

// scan_carry_kernel of a ragged call: one workgroup per stream s0 + blockIdx.x of a range whose streams with steps all have their
// last group in the chunk; a stream without steps in between returns at once.  The window is that of the stream's last live slot,
// step_off[s + 1] - 1 - p0 (the slots are compact); the tail comes from the stream's own packed samples.
template <bool PLANES>
__global__ __launch_bounds__(256) void scan_carry_ragged_kernel(const ScanChunkArgs a) {
    __shared__ float s_tail[kMaxTail];
    const int64_t s = a.s0 + blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t first = a.step_off[s], m = a.step_off[s + 1] - first;
    if (m == 0) return;
    const int64_t b = first + m - 1 - a.p0;
    const int64_t L = m * a.k_hop;
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
    const float* src = a.samples + first * a.k_hop;
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
template <bool CARRIED, bool RAGGED = false>
__global__ __launch_bounds__(256) void scan_smooth_kernel(const ScanDetectArgs a) {
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

// A ragged call (tcr_scan_ragged): the host's step offsets [N + 1] and the device tables [2][N + 1] (step offsets, then group
// offsets) at the front of the workspace.  Null in scan_run: the dense layout.
struct ScanRagged {
    const int64_t* step_off;    // host
    int64_t* tables;            // device
};

size_t scan_ragged_tables_bytes(int64_t n_signals) { return (size_t)round_up64(2 * (n_signals + 1) * (int64_t)sizeof(int64_t), 256); }

// Front-end frames of the call at group size G: every group is a row of G k + T - k frames, whatever its live steps.
int64_t scan_ragged_frames(const int64_t* so, int n_signals, int k, int T, int G) {
    int64_t rows = 0;
    for (int n = 0; n < n_signals; ++n) rows += ceil_div64(so[n + 1] - so[n], G);
    return rows * ((int64_t)G * k + T - k);
}

// The ragged chunking: G, at most kScanGroup, the longest signal and what one row of the workspace holds, with the fewest front-end
// frames over the call (ties: the larger G, fewer rows) -- the results do not depend on G, so this is a cost choice only; the sum is
// evaluated for every candidate while N x candidates stays small, for every few otherwise -- then R as scan_chunking finds it.
int scan_ragged_chunking(const tcr_frontend_cfg& cfg, const tcr_model_ref& m, const ModelIO& io, int k, const int64_t* so, int n_signals,
                         size_t ws_bytes, const char* what, ScanGeom& out) {
    const auto fits = [&](int G, int64_t R) {
        return scan_geom_ok(k, cfg.n_frames, G, R, io.max_batch) && (size_t)scan_geom(cfg, m, io, k, G, (int)R).ws_floats * sizeof(float) <= ws_bytes;
    };
    if (!fits(1, 1)) {
        set_error("%s: workspace %zu bytes < one window's %zu", what, ws_bytes, (size_t)scan_geom(cfg, m, io, k, 1, 1).ws_floats * sizeof(float));
        return TCR_ERR_WORKSPACE;
    }
    int64_t longest = 1;
    for (int n = 0; n < n_signals; ++n) longest = std::max(longest, so[n + 1] - so[n]);
    int lo = 1, hi = (int)std::min<int64_t>(kScanGroup, longest);      // the largest G one row of which fits (the size grows with G)
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (fits(mid, 1)) lo = mid;
        else hi = mid - 1;
    }
    const int g_max = lo;
    const int stride = (int)std::max<int64_t>(1, ceil_div64((int64_t)n_signals * g_max, (int64_t)1 << 22));
    int G = g_max;
    int64_t best = scan_ragged_frames(so, n_signals, k, cfg.n_frames, G);
    for (int c = g_max - stride; c >= 1; c -= stride) {
        const int64_t f = scan_ragged_frames(so, n_signals, k, cfg.n_frames, c);
        if (f < best) { best = f; G = c; }
    }
    int64_t total_groups = 0;
    for (int n = 0; n < n_signals; ++n) total_groups += ceil_div64(so[n + 1] - so[n], G);
    int64_t rlo = 1, rhi = total_groups;
    while (rlo < rhi) {
        const int64_t mid = (rlo + rhi + 1) / 2;
        if (fits(G, mid)) rlo = mid;
        else rhi = mid - 1;
    }
    out = scan_geom(cfg, m, io, k, G, (int)rlo);
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

// scan_run's ragged arm: the same stages over chunks of flattened groups, with the prefix tables in place of q / groups and
// n steps + i.  A chunk's live steps are the packed steps p(q0) .. p(q0 + rows) - 1 (a signal's groups cover its steps in order), so
// its windows are gathered compactly, the network runs at the batch of its live steps and writes their rows of the caller's logits
// and probs itself: no scatter.  The slots past a signal's last step cost front-end frames only.  With a state st
// (tcr_stream_scan_ragged) the signals are its streams: the carried forms of the stages, and after a chunk's gather the write-back
// of the streams whose last group is one of its rows (the header's state ordering).
int scan_run_ragged(const tcr_frontend_cfg& cfg, const void* plan_dev, const tcr_model_ref& m, const ModelIO& io, int n_signals, int k,
                    const tcr_detect_cfg& det, const float* samples, const ScanState& st, const ScanRagged& rg, void* workspace,
                    size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, hipStream_t s,
                    const char* what) {
    const int64_t* so = rg.step_off;
    ScanGeom g;
    TCR_TRY(scan_ragged_chunking(cfg, m, io, k, so, n_signals, ws_bytes, what, g));
    const int G = g.G;
    std::vector<int64_t> tables(2 * ((size_t)n_signals + 1));
    int64_t* go = tables.data() + n_signals + 1;
    std::copy(so, so + n_signals + 1, tables.data());
    go[0] = 0;
    for (int n = 0; n < n_signals; ++n) go[n + 1] = go[n] + ceil_div64(so[n + 1] - so[n], G);
    const int64_t total_groups = go[n_signals], total_steps = so[n_signals];
    // the tables live on the host's stack frame: the copy is complete before the call returns (and before the first launch)
    if (hipMemcpyAsync(rg.tables, tables.data(), tables.size() * sizeof(int64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: the upload of the offset tables failed", what);
        return TCR_ERR_HIP;
    }
    float* ws = static_cast<float*>(workspace);
    ScanChunkArgs ca{};
    ca.samples = samples; ca.stage = ws + g.stage_off; ca.frames = ws + g.frames_off; ca.windows = ws + g.win_off; ca.st = st;
    ca.k_hop = (int64_t)k * cfg.hop; ca.stride = g.stage_stride; ca.n_prefix = cfg.n_samples; ca.G = G; ca.k = k; ca.T = g.T; ca.tp = g.tp;
    ca.n_coef = g.n_coef; ca.ftp = tcr_padded_len(g.F); ca.step_off = rg.tables; ca.group_off = rg.tables + n_signals + 1; ca.n_sig = n_signals;
    const bool carried = st.window != nullptr;
    const auto gather = g.planes ? (carried ? scan_gather_kernel<true, true, true> : scan_gather_kernel<true, false, true>)
                                 : (carried ? scan_gather_kernel<false, true, true> : scan_gather_kernel<false, false, true>);
    int next = 0;                                       // carried: the first stream whose write-back is still to come
    // the packed step of flattened group q's first slot
    const auto first_step = [&](int64_t q) {
        if (q >= total_groups) return total_steps;
        const int64_t n = std::upper_bound(go, go + n_signals + 1, q) - go - 1;
        return so[n] + (q - go[n]) * G;
    };
    const int64_t stage_blocks = ceil_div64(g.stage_stride, 256);
    for (int64_t q0 = 0; q0 < total_groups; q0 += g.R) {
        const int rows = (int)std::min<int64_t>(g.R, total_groups - q0);
        ca.q0 = q0; ca.rows = rows; ca.p0 = first_step(q0);
        const int live = (int)(first_step(q0 + rows) - ca.p0);
        const int bx = (int)std::max<int64_t>(1, std::min(stage_blocks, ceil_div64(8 * (int64_t)device_cus(), rows)));
        if (carried) {
            hipLaunchKernelGGL(scan_stage_ragged_tail_kernel, dim3((unsigned)((int64_t)rows * bx)), dim3(256), 0, s, ca, bx);
            TCR_TRY(check_launch("scan_stage_ragged_tail_kernel"));
        } else {
            hipLaunchKernelGGL(scan_stage_ragged_kernel, dim3((unsigned)((int64_t)rows * bx)), dim3(256), 0, s, ca, bx);
            TCR_TRY(check_launch("scan_stage_ragged_kernel"));
        }
        TCR_TRY(stream_frontend(cfg, plan_dev, ca.stage, g.stage_stride, rows, g.F, ca.frames, s, ca.ftp));
        hipLaunchKernelGGL(gather, dim3(live), dim3(256), 0, s, ca);
        TCR_TRY(check_launch("scan_gather_kernel"));
        if (carried) {
            // the streams with steps whose last group (go[n + 1] - 1, increasing over them) is one of this chunk's rows: next .. the
            // last such one, streams without steps in between included (their workgroups return at once)
            int s_lo = -1, s_hi = -1;
            for (; next < n_signals && (so[next + 1] == so[next] || go[next + 1] - 1 < q0 + rows); ++next) {
                if (so[next + 1] == so[next]) continue;
                if (s_lo < 0) s_lo = next;
                s_hi = next;
            }
            if (s_lo >= 0) {
                ca.s0 = s_lo;
                if (g.planes) hipLaunchKernelGGL(scan_carry_ragged_kernel<true>, dim3((unsigned)(s_hi - s_lo + 1)), dim3(256), 0, s, ca);
                else hipLaunchKernelGGL(scan_carry_ragged_kernel<false>, dim3((unsigned)(s_hi - s_lo + 1)), dim3(256), 0, s, ca);
                TCR_TRY(check_launch("scan_carry_ragged_kernel"));
            }
        }
        TCR_TRY(model_forward(m, ca.windows, live, ws + g.net_off, ws_bytes - (size_t)g.net_off * sizeof(float), logits + ca.p0 * g.classes,
                              probs + ca.p0 * g.classes, s));
    }
    ScanDetectArgs da;
    da.probs = probs; da.smoothed = smoothed; da.top = top; da.score = score; da.is_new = is_new; da.st = st; da.steps = total_steps;
    da.N = n_signals; da.C = g.classes; da.W = det.average_steps; da.min_count = det.min_count; da.suppression = det.suppression_steps;
    da.threshold = det.threshold; da.step_off = rg.tables;
    if (carried) hipLaunchKernelGGL((scan_smooth_kernel<true, true>), dim3((unsigned)ceil_div64(total_steps, 256 / g.classes)), dim3(256), 0, s, da);
    else hipLaunchKernelGGL((scan_smooth_kernel<false, true>), dim3((unsigned)ceil_div64(total_steps, 256 / g.classes)), dim3(256), 0, s, da);
    TCR_TRY(check_launch("scan_smooth_kernel"));
    hipLaunchKernelGGL(scan_suppress_kernel<true>, dim3(n_signals), dim3(256), 0, s, da);
    return check_launch("scan_suppress_kernel");
}

// The pipeline of the header comment over n_signals x steps checked by the caller, from and to the state st (all null: none).
int scan_run(const tcr_frontend_cfg& cfg, const void* plan_dev, const tcr_model_ref& m, const ModelIO& io, int n_signals, int64_t steps,
             int k, const tcr_detect_cfg& det, const float* samples, const ScanState& st, void* workspace, size_t ws_bytes, float* logits,
             float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream, const char* what,
             const ScanRagged* rg = nullptr) {
    ScanGeom g;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rg) return scan_run_ragged(cfg, plan_dev, m, io, n_signals, k, det, samples, st, *rg, workspace, ws_bytes, logits, probs, smoothed,
                                   top, score, is_new, s, what);
    TCR_TRY(scan_chunking(cfg, m, io, k, steps, n_signals, ws_bytes, what, g));
    const int G = g.G;
    const int64_t groups = ceil_div64(steps, G), total_groups = groups * n_signals;
    float* ws = static_cast<float*>(workspace);
    ScanChunkArgs ca;
    ca.samples = samples; ca.stage = ws + g.stage_off; ca.frames = ws + g.frames_off; ca.windows = ws + g.win_off; ca.st = st;
    ca.k_hop = (int64_t)k * cfg.hop; ca.L = steps * ca.k_hop; ca.stride = g.stage_stride; ca.groups = groups; ca.steps = steps;
    ca.n_prefix = cfg.n_samples; ca.G = G; ca.k = k; ca.T = g.T; ca.tp = g.tp; ca.n_coef = g.n_coef; ca.ftp = tcr_padded_len(g.F);
    const bool carried = st.window != nullptr;
    const auto gather = g.planes ? (carried ? scan_gather_kernel<true, true> : scan_gather_kernel<true, false>)
                                 : (carried ? scan_gather_kernel<false, true> : scan_gather_kernel<false, false>);
    for (int64_t q0 = 0; q0 < total_groups; q0 += g.R) {
        const int rows = (int)std::min<int64_t>(g.R, total_groups - q0);
        const int slots = rows * G;
        ca.q0 = q0; ca.rows = rows;
        // the streams whose last group (s groups + groups - 1) is one of this chunk's rows
        const int64_t s_lo = (q0 + 1 + groups - 1) / groups - 1, s_hi = (q0 + rows) / groups - 1;
        ca.s0 = s_lo;
        const int64_t staged = (int64_t)rows * g.stage_stride;
        hipLaunchKernelGGL(scan_stage_kernel, dim3((unsigned)std::min<int64_t>(ceil_div64(staged, 256), 8 * (int64_t)device_cus())), dim3(256), 0,
                           s, ca);
        TCR_TRY(check_launch("scan_stage_kernel"));
        TCR_TRY(stream_frontend(cfg, plan_dev, ca.stage, g.stage_stride, rows, g.F, ca.frames, s, ca.ftp));
        hipLaunchKernelGGL(gather, dim3(slots), dim3(256), 0, s, ca);
        TCR_TRY(check_launch("scan_gather_kernel"));
        if (carried && s_hi >= s_lo) {
            if (g.planes) hipLaunchKernelGGL(scan_carry_kernel<true>, dim3((unsigned)(s_hi - s_lo + 1)), dim3(256), 0, s, ca);
            else hipLaunchKernelGGL(scan_carry_kernel<false>, dim3((unsigned)(s_hi - s_lo + 1)), dim3(256), 0, s, ca);
            TCR_TRY(check_launch("scan_carry_kernel"));
        }
        TCR_TRY(model_forward(m, ca.windows, slots, ws + g.net_off, ws_bytes - (size_t)g.net_off * sizeof(float), ws + g.logits_off,
                              ws + g.probs_off, stream));
        ScanScatterArgs xa;
        xa.logits_in = ws + g.logits_off; xa.probs_in = ws + g.probs_off; xa.logits = logits; xa.probs = probs; xa.q0 = q0;
        xa.groups = groups; xa.steps = steps; xa.G = G; xa.C = g.classes; xa.slots = slots;
        hipLaunchKernelGGL(scan_scatter_kernel, dim3(ceil_div(slots * g.classes, 256)), dim3(256), 0, s, xa);
        TCR_TRY(check_launch("scan_scatter_kernel"));
    }
    ScanDetectArgs da;
    da.probs = probs; da.smoothed = smoothed; da.top = top; da.score = score; da.is_new = is_new; da.st = st; da.steps = steps;
    da.N = n_signals; da.C = g.classes; da.W = det.average_steps; da.min_count = det.min_count; da.suppression = det.suppression_steps;
    da.threshold = det.threshold; da.step_off = nullptr;
    hipLaunchKernelGGL(carried ? scan_smooth_kernel<true> : scan_smooth_kernel<false>, dim3((unsigned)ceil_div64(n_signals * steps, 256 / g.classes)),
                       dim3(256), 0, s, da);
    TCR_TRY(check_launch("scan_smooth_kernel"));
    hipLaunchKernelGGL(scan_suppress_kernel<false>, dim3(n_signals), dim3(256), 0, s, da);
    return check_launch("scan_suppress_kernel");
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
    return scan_run(*cfg, plan_dev, *m, io, n_signals, steps, k, *det, samples, ScanState{}, workspace, ws_bytes, logits, probs, smoothed,
                    top, score, is_new, stream, what);
}

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
    TCR_REQUIRE((int64_t)n_streams * steps * io.classes < ((int64_t)1 << 31), "%s: %d streams x %lld steps is too large", what, n_streams,
                (long long)steps);
    const StreamGeom sg = stream_geom(*cfg, *m, io, n_streams, k, det->average_steps);
    float* st = static_cast<float*>(state);
    const ScanState carried{st + sg.win_off, st + sg.tail_off, st + sg.ring_off, reinterpret_cast<int*>(st + sg.ist_off), reset, sg.tail_len};
    return scan_run(*cfg, plan_dev, *m, io, n_streams, steps, k, *det, samples, carried, workspace, ws_bytes, logits, probs, smoothed, top,
                    score, is_new, stream, what);
}

int scan_ragged(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* m, int n_signals, const int64_t* sample_offsets,
                int k, const tcr_detect_cfg* det, const float* samples, void* workspace, size_t ws_bytes, float* logits, float* probs,
                float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream, const char* what) {
    TCR_REQUIRE(plan_dev && m && m->params && m->aux && det && sample_offsets && workspace, "%s: null argument", what);
    TCR_REQUIRE(n_signals > 0, "%s: the number of signals must be positive (got %d)", what, n_signals);
    ModelIO io;
    TCR_TRY(stream_check(cfg, m, n_signals, k, det, what, io, false));
    const size_t tables_bytes = scan_ragged_tables_bytes(n_signals);
    TCR_REQUIRE(tables_bytes <= ws_bytes, "%s: %d signals are more than the max_signals the workspace's offset tables hold (%lld)", what,
                n_signals, (long long)(ws_bytes / (2 * sizeof(int64_t))) - 1);
    const int64_t khop = (int64_t)k * cfg->hop;
    TCR_REQUIRE(sample_offsets[0] == 0, "%s: sample_offsets must start at 0 (got %lld)", what, (long long)sample_offsets[0]);
    std::vector<int64_t> so((size_t)n_signals + 1);
    so[0] = 0;
    for (int n = 0; n < n_signals; ++n) {
        const int64_t len = sample_offsets[n + 1] - sample_offsets[n];
        TCR_REQUIRE(len >= 0, "%s: sample_offsets decrease at signal %d (%lld after %lld)", what, n, (long long)sample_offsets[n + 1],
                    (long long)sample_offsets[n]);
        TCR_REQUIRE(len % khop == 0, "%s: the length %lld of signal %d is not a multiple of k * hop = %lld", what, (long long)len, n,
                    (long long)khop);
        so[n + 1] = so[n] + len / khop;
    }
    const int64_t total_steps = so[n_signals];
    TCR_REQUIRE(total_steps > 0, "%s: no signal has a whole step (total_steps == 0)", what);
    TCR_REQUIRE(total_steps * io.classes < ((int64_t)1 << 31), "%s: %lld steps in all is too large", what, (long long)total_steps);
    TCR_REQUIRE(samples && logits && probs && smoothed && top && score && is_new, "%s: null argument", what);
    const ScanRagged rg{so.data(), static_cast<int64_t*>(workspace)};
    return scan_run(*cfg, plan_dev, *m, io, n_signals, 0, k, *det, samples, ScanState{}, static_cast<char*>(workspace) + tables_bytes,
                    ws_bytes - tables_bytes, logits, probs, smoothed, top, score, is_new, stream, what, &rg);
}

// tcr_stream_scan_ragged: scan_ragged's checks with the streams of a state in place of fresh signals (a stream without steps is
// allowed, a call without any step is not), then the ragged pipeline from and to the state.
int stream_scan_ragged(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* m, int n_streams, const int64_t* sample_offsets,
                       int k, const tcr_detect_cfg* det, const float* samples, const uint8_t* reset, void* state, void* workspace,
                       size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream,
                       const char* what) {
    TCR_REQUIRE(plan_dev && m && m->params && m->aux && det && sample_offsets && state && workspace, "%s: null argument", what);
    ModelIO io;
    TCR_TRY(stream_check(cfg, m, n_streams, k, det, what, io));
    const size_t tables_bytes = scan_ragged_tables_bytes(n_streams);
    TCR_REQUIRE(tables_bytes <= ws_bytes, "%s: %d streams are more than the max_signals the workspace's offset tables hold (%lld)", what,
                n_streams, (long long)(ws_bytes / (2 * sizeof(int64_t))) - 1);
    const int64_t khop = (int64_t)k * cfg->hop;
    TCR_REQUIRE(sample_offsets[0] == 0, "%s: sample_offsets must start at 0 (got %lld)", what, (long long)sample_offsets[0]);
    std::vector<int64_t> so((size_t)n_streams + 1);
    so[0] = 0;
    for (int n = 0; n < n_streams; ++n) {
        const int64_t len = sample_offsets[n + 1] - sample_offsets[n];
        TCR_REQUIRE(len >= 0, "%s: sample_offsets decrease at stream %d (%lld after %lld)", what, n, (long long)sample_offsets[n + 1],
                    (long long)sample_offsets[n]);
        TCR_REQUIRE(len % khop == 0, "%s: the length %lld of stream %d is not a multiple of k * hop = %lld", what, (long long)len, n,
                    (long long)khop);
        so[n + 1] = so[n] + len / khop;
    }
    const int64_t total_steps = so[n_streams];
    TCR_REQUIRE(total_steps > 0, "%s: no stream has a whole step (total_steps == 0)", what);
    TCR_REQUIRE(total_steps * io.classes < ((int64_t)1 << 31), "%s: %lld steps in all is too large", what, (long long)total_steps);
    TCR_REQUIRE(samples && logits && probs && smoothed && top && score && is_new, "%s: null argument", what);
    const StreamGeom sg = stream_geom(*cfg, *m, io, n_streams, k, det->average_steps);
    float* st = static_cast<float*>(state);
    const ScanState carried{st + sg.win_off, st + sg.tail_off, st + sg.ring_off, reinterpret_cast<int*>(st + sg.ist_off), reset, sg.tail_len};
    const ScanRagged rg{so.data(), static_cast<int64_t*>(workspace)};
    return scan_run(*cfg, plan_dev, *m, io, n_streams, 0, k, *det, samples, carried, static_cast<char*>(workspace) + tables_bytes,
                    ws_bytes - tables_bytes, logits, probs, smoothed, top, score, is_new, stream, what, &rg);
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_stream_scan_ragged(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_net* net, const float* params,
                                      const float* frozen_ss, int n_streams, const int64_t* sample_offsets, int k, const tcr_detect_cfg* det,
                                      const float* samples, const uint8_t* reset, void* state, void* workspace, size_t ws_bytes,
                                      float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                                      void* stream) {
    const tcr_model_ref m = tcresnet_ref(net, params, frozen_ss);
    return stream_scan_ragged(cfg, plan_dev, &m, n_streams, sample_offsets, k, det, samples, reset, state, workspace, ws_bytes, logits, probs,
                              smoothed, top, score, is_new, stream, "tcr_stream_scan_ragged");
}

extern "C" int tcr_stream_scan_ragged_m(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_streams,
                                        const int64_t* sample_offsets, int k, const tcr_detect_cfg* det, const float* samples,
                                        const uint8_t* reset, void* state, void* workspace, size_t ws_bytes, float* logits, float* probs,
                                        float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    return stream_scan_ragged(cfg, plan_dev, model, n_streams, sample_offsets, k, det, samples, reset, state, workspace, ws_bytes, logits,
                              probs, smoothed, top, score, is_new, stream, "tcr_stream_scan_ragged_m");
}

extern "C" size_t tcr_scan_ragged_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int k, int max_windows,
                                                  int max_signals) {
    const size_t chunk = scan_workspace_bytes(cfg, model, k, max_windows, "tcr_scan_ragged_workspace_bytes");
    if (chunk == 0) return 0;
    if (max_signals < 1) { set_error("tcr_scan_ragged_workspace_bytes: max_signals must be >= 1 (got %d)", max_signals); return 0; }
    return scan_ragged_tables_bytes(max_signals) + chunk;
}

extern "C" int tcr_scan_ragged(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_signals,
                               const int64_t* sample_offsets, int k, const tcr_detect_cfg* det, const float* samples, void* workspace,
                               size_t ws_bytes, float* logits, float* probs, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                               void* stream) {
    return scan_ragged(cfg, plan_dev, model, n_signals, sample_offsets, k, det, samples, workspace, ws_bytes, logits, probs, smoothed, top,
                       score, is_new, stream, "tcr_scan_ragged");
}

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
