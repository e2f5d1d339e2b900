// Detector tuning from stored probabilities: the detector tail of a scan, run again on the probs [steps][C] a scan wrote.
//
//   tcr_detect_redetect(_ragged)  the fresh (no state) instances of scan_smooth_kernel and scan_suppress_kernel (scan.hip) on the
//                                 caller's arrays: bitwise the smoothed / top / score / is_new of a scan with this det.  Nothing is
//                                 copied and nothing is waited for (the ragged offsets are a device table), so the call can be
//                                 captured into a graph.
//   tcr_detect_grid               J points (W, min_count, suppression) x T thresholds in one call.  top / score depend on (W, min_count)
//                                 only, and the smoothing on W only, so the points are reduced to their distinct pairs, sorted by W:
//     grid_smooth_kernel          a workgroup per tile of TCR_GRID_TILE consecutive steps of one signal stages the tile's rows of probs
//                                 and the h = min(W_max - 1, first step of the tile) rows in front of them into LDS once (rows before
//                                 the signal's first step are never read), then per distinct W smooths every (step, class) of the
//                                 tile from LDS -- smooth_mean (stream.hip) over count = min(i + 1, W) rows, oldest first: the scan's
//                                 expression, so the rows are bitwise a scan's -- takes the argmax (lowest index on ties) and writes
//                                 top / score once per pair of that W with the pair's min_count gate, into workspace rows
//                                 [pair][total_steps].  Lanes map as in scan_smooth_kernel, a lane per (step, class), 256 / C steps a
//                                 pass: consecutive lanes read consecutive LDS floats (no bank conflict while count = W).
//     sweep_kernel (sweep.hip)    launched once per point on its pair's rows with the point's suppression_steps: the counts are
//                                 tcr_detect_sweep's by construction.
//   Ragged tiles without a host copy of the offsets: signal n's tiles are blocks f(n) .. with f(n) = step_off[n] / TILE + n, which
//   increases by at least the signal's ceil(len / TILE) tiles, so floor(total / TILE) + N blocks cover every tile; a block finds its
//   signal by binary search over f and returns when its tile lies past the signal's last step (a signal without steps has none).
//
// The LDS limit: (TCR_GRID_TILE + W_max - 1) x C floats of dynamic LDS plus the 1 KB argmax exchange stay within 64 KB a workgroup,
// i.e. W_max(C) = 16128 / C - 255 (C = 12: 1089, C = 3: 5121, C = 36: 193; none from C = 63 on).  Pairs whose W is above it take the
// per-pair path: detect_smooth_kernel<.., kSmoothTopScore> (scan_smooth_kernel's body) into the same workspace rows, one launch per
// pair, reading each row W times from L2 / HBM instead of LDS.  The tile of 256 steps keeps the halo's share of the staging at
// (W - 1) / 256 (19 % at the default W = 50) and the LDS at 15.3 KB for C = 12, W = 50: ten workgroups a CU by LDS, so the eight
// waves a SIMD the registers allow stay the bound.
//
// Workspace: per pair two rows (top int32, score float32) of total_steps, each rounded up to 256 bytes; tcr_detect_grid_workspace_bytes
// sizes it for n_points pairs.  With fewer bytes the pairs run in batches that fit (a W cut by a batch boundary is smoothed in both).
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after sweep.hip).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

namespace tcr {

namespace {

constexpr int kGridTile = TCR_GRID_TILE;
constexpr int kGridMaxPairs = 32;                       // pairs (and distinct W) per launch of grid_smooth_kernel
constexpr int kGridLdsFloats = (64 * 1024 - 256 * 4) / 4;      // dynamic LDS floats next to s_sm

// the largest W the LDS-staged kernel takes at C classes (< 1: none)
int grid_w_max(int C) { return kGridLdsFloats / C - (kGridTile - 1); }

}  // namespace

struct GridArgs {
    const float* probs;         // [N][steps][C] (ragged: packed)
    int32_t* top;               // rows [slot][row_stride] of the workspace
    float* score;
    int64_t row_stride;         // elements between a slot's row and the next slot's (top and score alike)
    int64_t steps, tiles;       // dense: steps and tiles per signal
    const int64_t* step_off;    // ragged: [N + 1]
    int N, C, halo;             // halo = the launch's largest W - 1
    int n_w;                    // distinct W of the launch; the pairs of w[k] are slots w_begin[k] .. w_begin[k + 1] - 1
    int w[kGridMaxPairs], w_begin[kGridMaxPairs + 1], min_count[kGridMaxPairs];
};

// Dynamic LDS: the staged rows [h + len][C].  33 VGPRs, no scratch (eight waves a SIMD); LDS = 1 KB + (TCR_GRID_TILE + W - 1) x C x 4
// bytes for the launch's largest W (15.3 KB at C = 12, W = 50).
template <bool RAGGED>
__global__ __launch_bounds__(256) void grid_smooth_kernel(const GridArgs a) {
    __shared__ float s_sm[256];
    float* s_p = reinterpret_cast<float*>(dyn_lds());
    const int tid = threadIdx.x, C = a.C;
    int64_t row0, i0, len_sig;
    if constexpr (RAGGED) {
        const int64_t b = blockIdx.x;
        int lo = 0, hi = a.N - 1;                       // the last n with step_off[n] / TILE + n <= b
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.step_off[mid] / kGridTile + mid <= b) lo = mid;
            else hi = mid - 1;
        }
        row0 = a.step_off[lo];
        len_sig = a.step_off[lo + 1] - row0;
        i0 = (b - (row0 / kGridTile + lo)) * kGridTile;
    } else {
        const int64_t n = blockIdx.x / (uint64_t)a.tiles;
        row0 = n * a.steps;
        len_sig = a.steps;
        i0 = (blockIdx.x - n * a.tiles) * kGridTile;
    }
    if (i0 >= len_sig) return;                          // (ragged: a signal without steps, or a spare block)
    const int len = (int)(len_sig - i0 < kGridTile ? len_sig - i0 : kGridTile);
    const int h = (int)(i0 < a.halo ? i0 : a.halo);     // rows in front of the tile (never before the signal's first)
    const float* src = a.probs + (row0 + i0 - h) * C;
    const int n_stage = (h + len) * C;
    for (int e = tid; e < n_stage; e += 256) s_p[e] = src[e];
    __syncthreads();
    const int per = 256 / C;
    const int ls = tid / C, c = tid - ls * C;
    const int passes = (len + per - 1) / per;
    for (int k = 0; k < a.n_w; ++k) {
        const int W = a.w[k];
        for (int p = 0; p < passes; ++p) {
            const int j = p * per + ls;                 // step of the tile
            const bool live = ls < per && j < len;
            int count = 0;
            if (live) {
                const int64_t i = i0 + j;
                count = i + 1 < W ? (int)(i + 1) : W;
                const float* q = s_p + (h + j - count + 1) * C + c;
                const float v = smooth_mean(count, [&]() {
                    const float x = *q;
                    q += C;
                    return x;
                });
                s_sm[tid] = v;
            }
            __syncthreads();
            if (live && c == 0) {
                int best = 0;
                float best_v = s_sm[tid];
                for (int cc = 1; cc < C; ++cc) {
                    const float v = s_sm[tid + cc];
                    if (v > best_v) { best = cc; best_v = v; }
                }
                const int64_t at = row0 + i0 + j;
                for (int s = a.w_begin[k]; s < a.w_begin[k + 1]; ++s) {
                    const bool warm = count >= a.min_count[s];
                    a.top[s * a.row_stride + at] = warm ? best : -1;
                    a.score[s * a.row_stride + at] = warm ? best_v : 0.f;
                }
            }
            __syncthreads();                            // (the next pass rewrites s_sm)
        }
    }
}

// scan_smooth_kernel's fresh instance (scan.hip: the same body) with the outputs a caller of these entries may leave out
template <bool RAGGED, int OUTS>
__global__ __launch_bounds__(256) void detect_smooth_kernel(const ScanDetectArgs a) {
    scan_smooth<false, RAGGED, OUTS>(a);
}

namespace {

// the refusals the two families share about one detector setting (stream_check's, with its messages)
int detect_point_check(const char* what, int W, int min_count, int suppression) {
    TCR_REQUIRE(W >= 1, "%s: average_steps (the ring of probability vectors) must be >= 1 (got %d)", what, W);
    TCR_REQUIRE(min_count >= 1 && min_count <= W, "%s: min_count %d outside 1..average_steps = %d", what, min_count, W);
    TCR_REQUIRE(suppression >= 0, "%s: suppression_steps must be >= 0 (got %d)", what, suppression);
    return TCR_OK;
}

// n_signals, steps (dense) / total_steps (ragged) and num_classes of a probs array
int detect_shape_check(const char* what, bool ragged, int n_signals, int64_t steps, int64_t total_steps, int num_classes) {
    TCR_TRY(detect_rows_check(what, ragged, n_signals, steps, total_steps, "signals"));
    TCR_REQUIRE(num_classes > 0 && num_classes <= kSweepMaxClasses, "%s: num_classes %d outside 1..%d", what, num_classes, kSweepMaxClasses);
    const int64_t rows = ragged ? total_steps : steps * n_signals;
    TCR_REQUIRE((ragged || steps < ((int64_t)1 << 31)) && rows < ((int64_t)1 << 31) && rows * num_classes < ((int64_t)1 << 31),
                "%s: %lld steps in all x %d classes is too large", what, (long long)rows, num_classes);
    return TCR_OK;
}

// the smoothing over probs with the outputs OUTS of the launch's da: the scan's own fresh kernel where every output is written
template <int OUTS>
int smooth_launch(const ScanDetectArgs& da, bool ragged, int64_t total_steps, hipStream_t s) {
    auto smooth = ragged ? detect_smooth_kernel<true, OUTS> : detect_smooth_kernel<false, OUTS>;
    if (OUTS == kSmoothAll) smooth = ragged ? scan_smooth_kernel<false, true> : scan_smooth_kernel<false, false>;
    hipLaunchKernelGGL(smooth, dim3((unsigned)ceil_div64(total_steps, 256 / da.C)), dim3(256), 0, s, da);
    return check_launch("scan_smooth_kernel");
}

int redetect(const char* what, bool ragged, int n_signals, int64_t steps, const int64_t* step_offsets, int64_t total_steps, int num_classes,
             const float* probs, const tcr_detect_cfg* det, float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    TCR_REQUIRE((!ragged || step_offsets) && probs && det && top && score && is_new, "%s: null argument", what);
    TCR_TRY(detect_shape_check(what, ragged, n_signals, steps, total_steps, num_classes));
    TCR_TRY(detect_point_check(what, det->average_steps, det->min_count, det->suppression_steps));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ScanDetectArgs da;
    da.probs = probs; da.smoothed = smoothed; da.top = top; da.score = score; da.is_new = is_new; da.st = ScanState{};
    da.steps = ragged ? total_steps : steps; da.N = n_signals; da.C = num_classes; da.W = det->average_steps; da.min_count = det->min_count;
    da.suppression = det->suppression_steps; da.threshold = det->threshold; da.step_off = ragged ? step_offsets : nullptr;
    const int64_t rows = ragged ? total_steps : steps * n_signals;
    TCR_TRY(smoothed ? smooth_launch<kSmoothAll>(da, ragged, rows, s) : smooth_launch<kSmoothNoVector>(da, ragged, rows, s));
    return suppress_launch(da, ragged, s);
}

// The carried detector tail over posteriors (tcr_phrase_stream_push*, tcr_dtw_stream_push*): redetect's detector at one vector per
// decision, from the integers `ist` of a stream state.  Refuses what the tail cannot run (`noun`: what the posteriors are over) and fills
// `da`, in front of the caller's first launch (a refused call writes nothing); the caller then launches its posteriors,
// smooth_launch<kSmoothNoVector>(da, ..), what must lie behind the readers of its old state, and suppress_launch(da, ..).
int posterior_tail_args(const char* what, const char* noun, const tcr_detect_cfg* det, const uint8_t* reset, int* ist, const float* post,
                        int32_t* top, float* score, int32_t* is_new, bool ragged, int64_t steps, int64_t total_steps, const int64_t* step_off,
                        int n_streams, int num_classes, ScanDetectArgs& da) {
    TCR_REQUIRE(det->average_steps == 1 && det->min_count == 1,
                "%s: the detector over %s posteriors takes one vector per decision: average_steps and min_count must be 1 (got %d, %d)", what, noun,
                det->average_steps, det->min_count);
    TCR_REQUIRE(det->suppression_steps >= 0, "%s: suppression_steps must be >= 0 (got %d)", what, det->suppression_steps);
    da.probs = post; da.smoothed = nullptr; da.top = top; da.score = score; da.is_new = is_new;
    da.st = ScanState{};
    da.st.window = reinterpret_cast<float*>(ist);       // (not read: non-null says that there is a state to start from)
    da.st.ist = ist; da.st.reset = reset;
    da.steps = ragged ? total_steps : steps; da.N = n_streams; da.C = num_classes; da.W = 1; da.min_count = 1;
    da.suppression = det->suppression_steps; da.threshold = det->threshold; da.step_off = ragged ? step_off : nullptr;
    return TCR_OK;
}

size_t grid_row_bytes(int64_t total_steps) { return (size_t)round_up64(total_steps * 4, 256); }

template <bool RAGGED>
int grid_smooth_launch(const GridArgs& a, unsigned blocks, hipStream_t s) {
    const size_t lds = (size_t)(kGridTile + a.halo) * a.C * sizeof(float);
    if (lds > 32 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(grid_smooth_kernel<RAGGED>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("tcr_detect_grid: hipFuncSetAttribute failed");
        return TCR_ERR_HIP;
    }
    hipLaunchKernelGGL(grid_smooth_kernel<RAGGED>, dim3(blocks), dim3(256), lds, s, a);
    return check_launch("grid_smooth_kernel");
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_detect_redetect(int n_signals, int64_t steps, int num_classes, const float* probs, const tcr_detect_cfg* det,
                                   float* smoothed, int32_t* top, float* score, int32_t* is_new, void* stream) {
    return redetect("tcr_detect_redetect", false, n_signals, steps, nullptr, 0, num_classes, probs, det, smoothed, top, score, is_new, stream);
}

extern "C" int tcr_detect_redetect_ragged(int n_signals, const int64_t* step_offsets, int64_t total_steps, int num_classes, const float* probs,
                                          const tcr_detect_cfg* det, float* smoothed, int32_t* top, float* score, int32_t* is_new,
                                          void* stream) {
    return redetect("tcr_detect_redetect_ragged", true, n_signals, 0, step_offsets, total_steps, num_classes, probs, det, smoothed, top, score,
                    is_new, stream);
}

extern "C" size_t tcr_detect_grid_workspace_bytes(int64_t total_steps, int n_points) {
    if (total_steps <= 0 || total_steps >= ((int64_t)1 << 31) || n_points <= 0) {
        set_error("tcr_detect_grid_workspace_bytes: total_steps %lld outside 1..2^31 - 1 or n_points %d < 1", (long long)total_steps, n_points);
        return 0;
    }
    return 2 * grid_row_bytes(total_steps) * (size_t)n_points;
}

extern "C" int tcr_detect_grid(int n_signals, int64_t steps, const int64_t* step_offsets, int64_t total_steps, int num_classes,
                               const float* probs, const int64_t* valid_steps, int n_points, const tcr_detect_point* points, int n_thresholds,
                               const float* thresholds, const int32_t* event_offsets, const int64_t* event_first, const int64_t* event_last,
                               const int32_t* event_label, int32_t* detections, int32_t* hits, int32_t* duplicates, void* workspace,
                               size_t ws_bytes, void* stream) {
    const char* what = "tcr_detect_grid";
    const bool ragged = step_offsets != nullptr;
    TCR_REQUIRE(probs && points && workspace, "%s: null argument", what);
    TCR_REQUIRE(n_points > 0, "%s: the number of points must be positive (got %d)", what, n_points);
    TCR_REQUIRE(!(ragged && valid_steps), "%s: valid_steps given together with step_offsets (the offsets are the lengths)", what);
    TCR_TRY(detect_shape_check(what, ragged, n_signals, steps, total_steps, num_classes));
    TCR_REQUIRE(ragged || total_steps == steps * n_signals, "%s: total_steps %lld is not n_signals x steps = %lld", what, (long long)total_steps,
                (long long)(steps * n_signals));
    // (top / score are the workspace's rows: any non-null pointer stands in for them here)
    TCR_TRY(sweep_check(what, ragged, n_signals, steps, step_offsets, num_classes, static_cast<const int32_t*>(workspace),
                        static_cast<const float*>(workspace), 0, n_thresholds, thresholds, event_offsets, event_first, event_last, event_label,
                        detections, hits, duplicates));
    for (int j = 0; j < n_points; ++j)
        TCR_TRY(detect_point_check(what, points[j].average_steps, points[j].min_count, points[j].suppression_steps));
    const int64_t table = (int64_t)n_signals * n_thresholds * num_classes;             // (< 2^31: sweep_check)
    TCR_REQUIRE((int64_t)n_points * table < ((int64_t)1 << 31), "%s: %d points x %d signals x %d thresholds x %d classes is too large", what,
                n_points, n_signals, n_thresholds, num_classes);
    // the distinct (W, min_count) pairs, sorted by W, and every point's pair
    std::vector<std::pair<int, int>> pairs((size_t)n_points);
    for (int j = 0; j < n_points; ++j) pairs[j] = {points[j].average_steps, points[j].min_count};
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    const size_t row_bytes = grid_row_bytes(total_steps), pair_bytes = 2 * row_bytes;
    if (ws_bytes < pair_bytes) {
        set_error("%s: workspace %zu bytes < one pair's rows %zu", what, ws_bytes, pair_bytes);
        return TCR_ERR_WORKSPACE;
    }
    const int n_pairs = (int)pairs.size();
    const int batch = (int)std::min<size_t>(ws_bytes / pair_bytes, (size_t)n_pairs);
    const int w_max = grid_w_max(num_classes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t* top = static_cast<int32_t*>(workspace);                                    // slot q: top at q pair_bytes, score a row behind
    float* score = reinterpret_cast<float*>(static_cast<char*>(workspace) + row_bytes);
    const int64_t stride = (int64_t)(pair_bytes / 4);
    for (int p0 = 0; p0 < n_pairs; p0 += batch) {
        const int p1 = std::min(n_pairs, p0 + batch);
        // the LDS-staged kernel over the batch's pairs within the limit, kGridMaxPairs a launch
        int q = p0;
        while (q < p1 && pairs[q].first <= w_max) {
            GridArgs a{};
            a.probs = probs; a.top = top + (q - p0) * stride; a.score = score + (q - p0) * stride; a.row_stride = stride;
            a.steps = steps; a.tiles = ragged ? 0 : ceil_div64(steps, kGridTile); a.step_off = step_offsets; a.N = n_signals; a.C = num_classes;
            int n = 0;
            for (; q < p1 && n < kGridMaxPairs && pairs[q].first <= w_max; ++q, ++n) {
                if (a.n_w == 0 || a.w[a.n_w - 1] != pairs[q].first) {
                    a.w[a.n_w] = pairs[q].first;
                    a.w_begin[a.n_w++] = n;
                }
                a.min_count[n] = pairs[q].second;
            }
            a.w_begin[a.n_w] = n;
            a.halo = a.w[a.n_w - 1] - 1;
            const int64_t blocks = ragged ? total_steps / kGridTile + n_signals : a.tiles * n_signals;
            TCR_TRY(ragged ? grid_smooth_launch<true>(a, (unsigned)blocks, s) : grid_smooth_launch<false>(a, (unsigned)blocks, s));
        }
        // above the limit: the scan's smoothing kernel, a launch per pair, into the same rows
        for (; q < p1; ++q) {
            ScanDetectArgs da{};
            da.probs = probs; da.top = top + (q - p0) * stride; da.score = score + (q - p0) * stride;
            da.steps = ragged ? total_steps : steps; da.N = n_signals; da.C = num_classes; da.W = pairs[q].first; da.min_count = pairs[q].second;
            da.step_off = step_offsets;
            TCR_TRY(smooth_launch<kSmoothTopScore>(da, ragged, total_steps, s));
        }
        // every point of the batch's pairs: the sweep over its pair's rows into its slice of the counts
        for (int j = 0; j < n_points; ++j) {
            const std::pair<int, int> key{points[j].average_steps, points[j].min_count};
            const int at = (int)(std::lower_bound(pairs.begin(), pairs.end(), key) - pairs.begin());
            if (at < p0 || at >= p1) continue;
            TCR_TRY(sweep(what, ragged, n_signals, steps, step_offsets, num_classes, top + (at - p0) * stride, score + (at - p0) * stride, valid_steps,
                          points[j].suppression_steps, n_thresholds, thresholds, event_offsets, event_first, event_last, event_label,
                          detections + j * table, hits ? hits + j * table : nullptr, duplicates ? duplicates + j * table : nullptr, nullptr,
                          stream));
        }
    }
    return TCR_OK;
}
