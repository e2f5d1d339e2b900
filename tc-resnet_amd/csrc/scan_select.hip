// Sparse scans and step selection: the two device halves of a cascade (a cheap model flags steps, an expensive one looks only there).
//
// tcr_scan_steps: the fresh ragged scan of scan.hip (tcr_scan_ragged) for a chosen subset of its packed steps, at the cost of that
// subset.  Row b of logits / probs is bitwise row selected[b] of tcr_scan_ragged's: a frame is a pure function of its samples and the
// network's result for a window does not depend on its batch (scan.hip), so nothing here depends on which other steps are computed.
// Steps are cut into groups of G steps of one signal exactly as there; only the LIVE groups -- those that hold a selected step -- are
// staged and run through the front-end, a group still being one row of F = G k + T - k frames.  The live groups in order are the live
// rows; a chunk is R consecutive live rows, and because `selected` is sorted and a signal's groups are in order, a chunk's slots are
// one contiguous range b0 .. b1 - 1 of `selected`:
//   steps_stage_kernel     the R rows, as scan_stage_ragged_kernel<false> (the same copy loop); a workgroup finds its row's group from
//                          the row table, which holds the first packed step of every live row's group (so its signal comes from the
//                          step offsets by ragged_signal and no group offsets are needed);
//   frontend_pk3_kernel    over R rows of F frames (stream_frontend);
//   steps_gather_kernel    <PLANES>: slot b is packed step selected[b0 + b]; its signal by ragged_signal, its row from the table, its
//                          column j k with j = step % G; the copy loops of scan_gather_kernel<PLANES, false, true>;
//   the network at the batch of the slots, which writes rows b0 .. of the caller's compact logits / probs itself -- no scatter.
// G is the group size with the fewest front-end frames summed over the live groups (ties: the larger); the live groups at a G are
// counted from the runs of consecutive selected steps, so the choice costs runs x candidates and not steps x candidates.  The tables
// (step offsets [N + 1], selected, every selected step's live row, every live row's first step; int64) are built by the host and
// uploaded once to the workspace's front, and the call waits for that copy as tcr_scan_ragged does.
//
// tcr_scan_select: which steps to look at.  Step p is flagged when a masked class has values[p][c] >= enter, and selected when a flagged
// step of its signal lies in p - pad_after .. p + pad_before.  Prefix sums over the packed steps, each in three phases (per-workgroup
// sums of tiles of kSelTile steps, a scan of those sums by one workgroup, then apply), once for the flags and once for the compaction:
//   select_flag_kernel     a lane per (step, class), as scan_smooth_kernel reads probs: the flag bytes;
//   select_count_kernel    a tile's count; select_scan_kernel: the exclusive scan of the tiles' counts (one workgroup, 256 a pass, a
//                          carry between passes);
//   select_prefix_kernel   prefix[p] = the flags in 0 .. p;
//   select_dilate_kernel   a lane per step: selected <=> prefix[hi] - prefix[lo - 1] > 0 over lo .. hi, the pad range clamped to the
//                          signal's rows (so a flag never reaches another signal); the bytes replace the flags (and go to `mask`);
//   select_count_kernel, select_scan_kernel (which writes n_selected), select_compact_kernel: the selected steps in increasing order.
// Linear in the steps, independent of the pads, no floating-point arithmetic, and no workgroup waits for another: every dependence
// between workgroups is a kernel boundary.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after detect_grid.hip).
#pragma once
#include <algorithm>
#include <vector>

namespace tcr {

namespace {

constexpr int kSelTile = 1024;          // steps per workgroup of the prefix phases: four consecutive steps per thread

}  // namespace

// a chunk: live rows r0 .. and the slots b0 .. of `selected` that lie in them
struct StepsChunkArgs {
    const float* samples;       // packed
    float* stage;               // [R][stride]
    float* frames;              // [R][n_coef][ftp]
    float* windows;             // [slots][n_coef][tp] (planes: [slots][T n_coef + 2 kHalo])
    const int64_t* step_off;    // [N + 1]
    const int64_t* selected;    // [n_selected]: packed steps, increasing
    const int64_t* row_of;      // [n_selected]: the live row of every selected step
    const int64_t* row_first;   // [live rows]: the first packed step of the row's group
    int64_t stride, r0, b0, n_prefix, k_hop;
    int G, k, T, tp, n_coef, ftp, n_sig;
};

// Staging row r = live row r0 + r: scan_stage_ragged_kernel<false>'s row of the group whose first packed step the table holds (step
// g G of its signal: x from sample (g G + 1) k hop of  zeros(n_prefix) ++ signal ++ zeros).  bx workgroups per row.
__global__ __launch_bounds__(256) void steps_stage_kernel(const StepsChunkArgs a, const int bx) {
    const int64_t r = blockIdx.x / (unsigned)bx;
    const int part = (int)(blockIdx.x - (unsigned)r * bx);
    const int64_t p = a.row_first[a.r0 + r];
    const int n = ragged_signal(a.step_off, a.n_sig, p);
    const int64_t first = a.step_off[n], len = (a.step_off[n + 1] - first) * a.k_hop;
    const float* src = a.samples + first * a.k_hop;
    const int64_t base = (p - first + 1) * a.k_hop - a.n_prefix;
    float* dst = a.stage + r * a.stride;
    for (int64_t x = (int64_t)part * 256 + threadIdx.x; x < a.stride; x += (int64_t)bx * 256) {
        const int64_t pos = base + x;
        float v = 0.f;
        if (pos >= 0 && pos < len) v = src[pos];
        dst[x] = v;
    }
}

// One workgroup per slot b = packed step selected[b0 + b]: window column t <- column j k + t of its live row's frames (j = its step
// within the group); the halo is zero.  PLANES: the same window in plane order (scan_gather_kernel).
template <bool PLANES>
__global__ __launch_bounds__(256) void steps_gather_kernel(const StepsChunkArgs a) {
    const int b = blockIdx.x;
    const int64_t p = a.selected[a.b0 + b];
    const int sig = ragged_signal(a.step_off, a.n_sig, p);
    const int64_t i = p - a.step_off[sig];
    const int j = (int)(i % a.G);
    const int r = (int)(a.row_of[a.b0 + b] - a.r0);
    const float* src = a.frames + (size_t)r * a.n_coef * a.ftp + j * a.k;
    if constexpr (PLANES) {
        const int n = a.T * a.n_coef, pp = n + 2 * kHalo;
        float* dst = a.windows + (size_t)b * pp;
        for (int e = threadIdx.x; e < pp; e += 256) {
            const int o = e - kHalo;
            float v = 0.f;
            if (o >= 0 && o < n) {
                const int t = o / a.n_coef, c = o - t * a.n_coef, x = t + kHalo;
                v = src[(size_t)c * a.ftp + x];
            }
            dst[e] = v;
        }
    } else {
        float* dst = a.windows + (size_t)b * a.n_coef * a.tp;
        const int n = a.n_coef * a.tp;
        const int dc = 256 / a.tp, dx = 256 - dc * a.tp;
        int c = threadIdx.x / a.tp, x = threadIdx.x - c * a.tp;
        for (int e = threadIdx.x; e < n; e += 256) {
            const int t = x - kHalo;
            dst[e] = t >= 0 && t < a.T ? src[(size_t)c * a.ftp + x] : 0.f;
            c += dc;
            x += dx;
            if (x >= a.tp) { x -= a.tp; ++c; }
        }
    }
}

struct SelectArgs {
    const float* values;        // [total][C]
    const uint8_t* class_mask;  // [C]
    const int64_t* step_off;    // [N + 1]
    uint8_t* bits;              // [total]: the flags, then the selection
    int32_t* prefix;            // [total]: the flags in 0 .. p
    int32_t* sums;              // [tiles + 1]: a tile's count, then the count in front of the tile (sums[tiles]: all)
    int64_t* selected;
    int64_t* n_selected;        // select_scan_kernel: written when not null
    uint8_t* mask;              // [total] or null
    int64_t total;
    int tiles, N, C, pad_before, pad_after;
    float enter;
};

// The exclusive prefix of v over the workgroup's 256 threads in thread order, and their sum.  Every thread calls it.
__device__ __forceinline__ int select_block_prefix(int v, int& total) {
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[w] = x;
    __syncthreads();
    int base = 0;
    for (int u = 0; u < w; ++u) base += s_wave[u];
    total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();                                                    // (the next call rewrites s_wave)
    return base + x - v;
}

// A lane per (step, class), 256 / C steps per workgroup; a float32 compare, so a NaN never flags.
__global__ __launch_bounds__(256) void select_flag_kernel(const SelectArgs a) {
    __shared__ int s_f[256];
    const int C = a.C, per = 256 / C;
    const int ls = threadIdx.x / C, c = threadIdx.x - ls * C;
    const int64_t p = (int64_t)blockIdx.x * per + ls;
    const bool live = ls < per && p < a.total;
    int f = 0;
    if (live) f = a.class_mask[c] != 0 && a.values[p * C + c] >= a.enter;
    s_f[threadIdx.x] = f;
    __syncthreads();
    if (!live || c != 0) return;
    for (int cc = 1; cc < C; ++cc) f |= s_f[threadIdx.x + cc];
    a.bits[p] = (uint8_t)f;
}

// the bytes of a thread's four consecutive steps of tile blockIdx.x (0 past the last step), and the first of them
__device__ __forceinline__ int64_t select_tile_bits(const SelectArgs& a, int (&v)[4]) {
    const int64_t at = (int64_t)blockIdx.x * kSelTile + threadIdx.x * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = at + e < a.total ? a.bits[at + e] : 0;
    return at;
}

__global__ __launch_bounds__(256) void select_count_kernel(const SelectArgs a) {
    int v[4], total;
    select_tile_bits(a, v);
    select_block_prefix(v[0] + v[1] + v[2] + v[3], total);
    if (threadIdx.x == 0) a.sums[blockIdx.x] = total;
}

// One workgroup: sums[t] <- the counts of the tiles in front of t, sums[tiles] <- all of them (n_selected too, when given).
__global__ __launch_bounds__(256) void select_scan_kernel(const SelectArgs a) {
    int carry = 0;
    for (int base = 0; base < a.tiles; base += 256) {
        const int t = base + threadIdx.x;
        const int v = t < a.tiles ? a.sums[t] : 0;
        int total;
        const int ex = select_block_prefix(v, total);
        if (t < a.tiles) a.sums[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        a.sums[a.tiles] = carry;
        if (a.n_selected) *a.n_selected = carry;
    }
}

__global__ __launch_bounds__(256) void select_prefix_kernel(const SelectArgs a) {
    int v[4], total;
    const int64_t at = select_tile_bits(a, v);
    int run = a.sums[blockIdx.x] + select_block_prefix(v[0] + v[1] + v[2] + v[3], total);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        run += v[e];
        if (at + e < a.total) a.prefix[at + e] = run;
    }
}

// A lane per step: the flags in the pad range, clamped to the signal's rows.
__global__ __launch_bounds__(256) void select_dilate_kernel(const SelectArgs a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t p = (int64_t)blockIdx.x * kSelTile + e * 256 + threadIdx.x;
        if (p >= a.total) continue;
        const int n = ragged_signal(a.step_off, a.N, p);
        const int64_t row0 = a.step_off[n], end = a.step_off[n + 1];
        const int64_t lo = p - a.pad_after > row0 ? p - a.pad_after : row0;
        const int64_t hi = p + a.pad_before < end - 1 ? p + a.pad_before : end - 1;
        const int count = a.prefix[hi] - (lo > 0 ? a.prefix[lo - 1] : 0);
        const uint8_t sel = count > 0 ? 1 : 0;
        a.bits[p] = sel;
        if (a.mask) a.mask[p] = sel;
    }
}

__global__ __launch_bounds__(256) void select_compact_kernel(const SelectArgs a) {
    int v[4], total;
    const int64_t at = select_tile_bits(a, v);
    int64_t out = a.sums[blockIdx.x] + select_block_prefix(v[0] + v[1] + v[2] + v[3], total);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (v[e]) a.selected[out++] = at + e;
}

namespace {

size_t steps_tables_bytes(int64_t n_signals, int64_t n_selected) {
    return (size_t)round_up64((n_signals + 1 + 3 * n_selected) * (int64_t)sizeof(int64_t), 256);
}

struct StepsRun { int n; int64_t a, b; };               // steps a .. b of signal n, all selected

// What a checked call runs: the chunk geometry and the host tables.
struct StepsPlan {
    ScanGeom g;
    int64_t rows;                                       // live rows
    std::vector<int64_t> tables;                        // step offsets | selected | row_of | row_first
};

// Checks of tcr_scan_steps and tcr_scan_steps_plan up to the plan (G by the fewest frames over the live groups, R by the bytes behind
// the tables).  n_selected == 0: TCR_OK with plan.rows = 0 and nothing else filled in.
int steps_plan(const char* what, const tcr_frontend_cfg* cfg, const tcr_model_ref* m, int N, const int64_t* sample_offsets, int k,
               const int64_t* selected, int64_t n_selected, size_t ws_bytes, StepsPlan& plan) {
    TCR_REQUIRE(sample_offsets, "%s: null argument", what);
    TCR_REQUIRE(N > 0, "%s: the number of signals must be positive (got %d)", what, N);
    ModelIO io;
    TCR_TRY(stream_check(cfg, m, N, k, nullptr, what, io, false));
    TCR_REQUIRE(n_selected >= 0, "%s: n_selected must be >= 0 (got %lld)", what, (long long)n_selected);
    const size_t tables_bytes = steps_tables_bytes(N, n_selected);
    TCR_REQUIRE(tables_bytes <= ws_bytes, "%s: %d signals and %lld selected steps are more than the max_signals and max_selected the "
                "workspace's tables hold (%zu bytes of %zu)", what, N, (long long)n_selected, tables_bytes, ws_bytes);
    std::vector<int64_t> so;
    TCR_TRY(scan_step_offsets(what, "signal", N, (int64_t)k * cfg->hop, io.classes, sample_offsets, so));
    TCR_REQUIRE(n_selected == 0 || selected, "%s: null selected with n_selected = %lld", what, (long long)n_selected);
    const int64_t total = so[N];
    for (int64_t b = 0; b < n_selected; ++b) {
        TCR_REQUIRE(selected[b] >= 0 && selected[b] < total, "%s: selected[%lld] = %lld outside 0..%lld", what, (long long)b,
                    (long long)selected[b], (long long)total - 1);
        TCR_REQUIRE(b == 0 || selected[b] > selected[b - 1], "%s: selected is not strictly increasing at %lld (%lld after %lld)", what,
                    (long long)b, (long long)selected[b], (long long)selected[b - 1]);
    }
    plan.rows = 0;
    if (n_selected == 0) return TCR_OK;
    // the runs of consecutive selected steps of one signal
    std::vector<StepsRun> runs;
    int64_t longest = 1;
    {
        int n = 0;
        for (int64_t b = 0; b < n_selected; ++b) {
            const int64_t p = selected[b];
            while (so[n + 1] <= p) ++n;
            const int64_t i = p - so[n];
            if (!runs.empty() && runs.back().n == n && runs.back().b + 1 == i) runs.back().b = i;
            else runs.push_back(StepsRun{n, i, i});
        }
        for (int q = 0; q < N; ++q) longest = std::max(longest, so[q + 1] - so[q]);
    }
    const size_t chunk_bytes = ws_bytes - tables_bytes;
    const int T = cfg->n_frames;
    const auto bytes = [&](int G, int64_t R) { return (size_t)scan_geom(*cfg, *m, io, k, G, (int)R).ws_floats * sizeof(float); };
    const auto fits = [&](int G, int64_t R) { return scan_geom_ok(k, T, G, R, io.max_batch) && bytes(G, R) <= chunk_bytes; };
    const auto largest = [](int64_t lo, int64_t hi, const auto& ok) {
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (ok(mid)) lo = mid;
            else hi = mid - 1;
        }
        return lo;
    };
    if (!fits(1, 1)) {
        set_error("%s: workspace %zu bytes < one window's %zu", what, chunk_bytes, bytes(1, 1));
        return TCR_ERR_WORKSPACE;
    }
    const auto live_rows = [&](int G) {
        int64_t rows = 0, last_g = -1;
        int last_n = -1;
        for (const StepsRun& r : runs) {
            const int64_t ga = r.a / G, gb = r.b / G;
            rows += gb - ga + 1 - (r.n == last_n && ga == last_g ? 1 : 0);
            last_n = r.n;
            last_g = gb;
        }
        return rows;
    };
    const int g_max = (int)largest(1, std::min<int64_t>(kScanGroup, longest), [&](int64_t g) { return fits((int)g, 1); });
    const auto frames = [&](int g) { return live_rows(g) * ((int64_t)g * k + T - k); };
    const int stride = (int)std::max<int64_t>(1, ceil_div64((int64_t)runs.size() * g_max, (int64_t)1 << 22));
    int G = g_max;
    int64_t best = frames(G);
    for (int g = g_max - stride; g >= 1; g -= stride) {
        const int64_t f = frames(g);
        if (f < best) { best = f; G = g; }
    }
    plan.rows = live_rows(G);
    plan.g = scan_geom(*cfg, *m, io, k, G, (int)largest(1, plan.rows, [&](int64_t R) { return fits(G, R); }));
    // the tables
    std::vector<int64_t>& t = plan.tables;
    t.resize((size_t)N + 1 + 2 * (size_t)n_selected + (size_t)plan.rows);
    std::copy(so.begin(), so.end(), t.begin());
    int64_t* sel = t.data() + N + 1;
    int64_t* row_of = sel + n_selected;
    int64_t* row_first = row_of + n_selected;
    std::copy(selected, selected + n_selected, sel);
    int64_t rows = 0, last_g = -1;
    int last_n = -1, n = 0;
    for (int64_t b = 0; b < n_selected; ++b) {
        const int64_t p = selected[b];
        while (so[n + 1] <= p) ++n;
        const int64_t g = (p - so[n]) / G;
        if (n != last_n || g != last_g) {
            row_first[rows++] = so[n] + g * G;
            last_n = n;
            last_g = g;
        }
        row_of[b] = rows - 1;
    }
    return TCR_OK;
}

int select_launch(const SelectArgs& a, hipStream_t s) {
    const int per = 256 / a.C;
    SelectArgs b = a;
    b.n_selected = nullptr;
    hipLaunchKernelGGL(select_flag_kernel, dim3((unsigned)ceil_div64(a.total, per)), dim3(256), 0, s, b);
    TCR_TRY(check_launch("select_flag_kernel"));
    hipLaunchKernelGGL(select_count_kernel, dim3(a.tiles), dim3(256), 0, s, b);
    TCR_TRY(check_launch("select_count_kernel"));
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, s, b);
    TCR_TRY(check_launch("select_scan_kernel"));
    hipLaunchKernelGGL(select_prefix_kernel, dim3(a.tiles), dim3(256), 0, s, b);
    TCR_TRY(check_launch("select_prefix_kernel"));
    hipLaunchKernelGGL(select_dilate_kernel, dim3(a.tiles), dim3(256), 0, s, b);
    TCR_TRY(check_launch("select_dilate_kernel"));
    hipLaunchKernelGGL(select_count_kernel, dim3(a.tiles), dim3(256), 0, s, b);
    TCR_TRY(check_launch("select_count_kernel"));
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, s, a);
    TCR_TRY(check_launch("select_scan_kernel"));
    hipLaunchKernelGGL(select_compact_kernel, dim3(a.tiles), dim3(256), 0, s, a);
    return check_launch("select_compact_kernel");
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" size_t tcr_scan_steps_workspace_bytes(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int k, int max_windows,
                                                 int max_signals, int64_t max_selected) {
    const char* what = "tcr_scan_steps_workspace_bytes";
    const size_t chunk = scan_workspace_bytes(cfg, model, k, max_windows, what);
    if (chunk == 0) return 0;
    if (max_signals < 1) { set_error("%s: max_signals must be >= 1 (got %d)", what, max_signals); return 0; }
    if (max_selected < 1) { set_error("%s: max_selected must be >= 1 (got %lld)", what, (long long)max_selected); return 0; }
    return steps_tables_bytes(max_signals, max_selected) + chunk;
}

extern "C" int tcr_scan_steps_plan(const tcr_frontend_cfg* cfg, const tcr_model_ref* model, int n_signals, const int64_t* sample_offsets,
                                   int k, const int64_t* selected, int64_t n_selected, size_t ws_bytes, int64_t* plan_out) {
    const char* what = "tcr_scan_steps_plan";
    TCR_REQUIRE(plan_out, "%s: null argument", what);
    StepsPlan plan;
    TCR_TRY(steps_plan(what, cfg, model, n_signals, sample_offsets, k, selected, n_selected, ws_bytes, plan));
    plan_out[0] = plan.rows ? plan.g.G : 0;
    plan_out[1] = plan.rows;
    plan_out[2] = plan.rows ? plan.g.F : 0;
    plan_out[3] = plan.rows ? plan.g.R : 0;
    return TCR_OK;
}

extern "C" int tcr_scan_steps(const tcr_frontend_cfg* cfg, const void* plan_dev, const tcr_model_ref* model, int n_signals,
                              const int64_t* sample_offsets, int k, const int64_t* selected, int64_t n_selected, const float* samples,
                              void* workspace, size_t ws_bytes, float* logits, float* probs, void* stream) {
    const char* what = "tcr_scan_steps";
    TCR_REQUIRE(plan_dev && model && model->params && model->aux && workspace, "%s: null argument", what);
    StepsPlan plan;
    TCR_TRY(steps_plan(what, cfg, model, n_signals, sample_offsets, k, selected, n_selected, ws_bytes, plan));
    if (n_selected == 0) return TCR_OK;
    TCR_REQUIRE(samples && logits && probs, "%s: null argument", what);
    const ScanGeom& g = plan.g;
    const int N = n_signals;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the tables live in this frame: the copy is complete before the call returns (and before the first launch)
    int64_t* tables = static_cast<int64_t*>(workspace);
    if (hipMemcpyAsync(tables, plan.tables.data(), plan.tables.size() * sizeof(int64_t), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        set_error("%s: the upload of the tables failed", what);
        return TCR_ERR_HIP;
    }
    const size_t tables_bytes = steps_tables_bytes(N, n_selected);
    float* ws = reinterpret_cast<float*>(static_cast<char*>(workspace) + tables_bytes);
    const size_t chunk_bytes = ws_bytes - tables_bytes;
    const int64_t* row_of = plan.tables.data() + N + 1 + n_selected;
    StepsChunkArgs ca{};
    ca.samples = samples; ca.stage = ws + g.stage_off; ca.frames = ws + g.frames_off; ca.windows = ws + g.win_off;
    ca.step_off = tables; ca.selected = tables + N + 1; ca.row_of = ca.selected + n_selected; ca.row_first = ca.row_of + n_selected;
    ca.stride = g.stage_stride; ca.n_prefix = cfg->n_samples; ca.k_hop = (int64_t)k * cfg->hop; ca.G = g.G; ca.k = k; ca.T = g.T; ca.tp = g.tp;
    ca.n_coef = g.n_coef; ca.ftp = tcr_padded_len(g.F); ca.n_sig = N;
    const auto gather = g.planes ? steps_gather_kernel<true> : steps_gather_kernel<false>;
    const int64_t stage_blocks = ceil_div64(g.stage_stride, 256);
    int64_t b0 = 0;
    for (int64_t r0 = 0; r0 < plan.rows; r0 += g.R) {
        const int rows = (int)std::min<int64_t>(g.R, plan.rows - r0);
        const int64_t b1 = std::lower_bound(row_of + b0, row_of + n_selected, r0 + rows) - row_of;
        const int slots = (int)(b1 - b0);
        ca.r0 = r0; ca.b0 = b0;
        const int bx = (int)std::max<int64_t>(1, std::min(stage_blocks, ceil_div64(8 * (int64_t)device_cus(), rows)));
        hipLaunchKernelGGL(steps_stage_kernel, dim3((unsigned)((int64_t)rows * bx)), dim3(256), 0, s, ca, bx);
        TCR_TRY(check_launch("steps_stage_kernel"));
        TCR_TRY(stream_frontend(*cfg, plan_dev, ca.stage, g.stage_stride, rows, g.F, ca.frames, s, ca.ftp));
        hipLaunchKernelGGL(gather, dim3(slots), dim3(256), 0, s, ca);
        TCR_TRY(check_launch("steps_gather_kernel"));
        TCR_TRY(model_forward(*model, ca.windows, slots, ws + g.net_off, chunk_bytes - (size_t)g.net_off * sizeof(float),
                              logits + b0 * g.classes, probs + b0 * g.classes, stream));
        b0 = b1;
    }
    return TCR_OK;
}

extern "C" size_t tcr_scan_select_workspace_bytes(int64_t total_steps) {
    if (total_steps <= 0 || total_steps >= ((int64_t)1 << 31)) {
        set_error("tcr_scan_select_workspace_bytes: total_steps %lld outside 1..2^31 - 1", (long long)total_steps);
        return 0;
    }
    const int64_t tiles = ceil_div64(total_steps, kSelTile);
    return (size_t)(round_up64(total_steps, 256) + round_up64(total_steps * 4, 256) + round_up64((tiles + 1) * 4, 256));
}

extern "C" int tcr_scan_select(int n_signals, const int64_t* step_offsets, int64_t total_steps, int num_classes, const float* values,
                               const uint8_t* class_mask, float enter, int pad_before, int pad_after, void* workspace, size_t ws_bytes,
                               int64_t* selected, int64_t* n_selected, uint8_t* mask, void* stream) {
    const char* what = "tcr_scan_select";
    TCR_REQUIRE(step_offsets && values && class_mask && workspace && selected && n_selected, "%s: null argument", what);
    TCR_TRY(detect_shape_check(what, true, n_signals, 0, total_steps, num_classes));
    TCR_REQUIRE(enter == enter, "%s: enter is NaN", what);
    TCR_REQUIRE(pad_before >= 0 && pad_after >= 0, "%s: the pads must be >= 0 (got %d before, %d after)", what, pad_before, pad_after);
    const size_t need = tcr_scan_select_workspace_bytes(total_steps);
    if (ws_bytes < need) {
        set_error("%s: workspace %zu bytes < %zu for %lld steps", what, ws_bytes, need, (long long)total_steps);
        return TCR_ERR_WORKSPACE;
    }
    SelectArgs a{};
    a.values = values; a.class_mask = class_mask; a.step_off = step_offsets;
    a.bits = static_cast<uint8_t*>(workspace);
    a.prefix = reinterpret_cast<int32_t*>(a.bits + round_up64(total_steps, 256));
    a.sums = a.prefix + round_up64(total_steps * 4, 256) / 4;
    a.selected = selected; a.n_selected = n_selected; a.mask = mask; a.total = total_steps;
    a.tiles = (int)ceil_div64(total_steps, kSelTile); a.N = n_signals; a.C = num_classes; a.pad_before = pad_before; a.pad_after = pad_after;
    a.enter = enter;
    return select_launch(a, static_cast<hipStream_t>(stream));
}
