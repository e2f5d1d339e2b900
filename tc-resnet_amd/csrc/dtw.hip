// Enrolled keywords by template matching (tcr_dtw_scores, tcr_dtw_scores_ragged): rows [steps][F] of float32 features in (a scan's
// posteriors), out [steps][K + 1] posteriors over K enrolled keywords and a background class -- per keyword the best of its
// templates' confidences, a template's confidence 1 - scale x the cost of the best subsequence-DTW path that ends at the step -- and
// lengths [steps][K], the steps that path spans, so that the detector, sweep, grid and mining entries apply to enrolled keywords with
// num_classes = K + 1.  The contract (include/tcresnet_hip.h) fixes the float32 operations and their order; the kernel evaluates
// exactly those (no multiply-add is fused: fp contract(off) in every function that computes).
//
// The recurrence reads the previous column only -- D[j] = d(j, t) + min(D'[j - 1], D'[j], D'[j - 2]) -- so a step has no dependency
// along the template and a walk is sequential in t alone.
//
//   dtw_kernel       The layout chosen: ONE WAVE PER (SIGNAL, KEYWORD), a workgroup of 64 threads, grid (N, K).  The wave walks the
//                    keyword's templates one after the other, each over all of the signal's rows.  For a template of L frames a lane
//                    owns FPL = ceil(L / 64) consecutive frames (one fully unrolled instance per FPL 1 .. 4, chosen by a uniform
//                    switch; D and n of the lane's frames in registers, no scratch); frames past L compute on zeros and are never read
//                    by a frame below L.  The lane's template frames sit in dynamic LDS, feature-major and lane-minor
//                    (s_T[(i F + f) 64 + lane]: conflict-free, and private to the lane, so no barrier guards them).  The signal's rows
//                    come through a tile of kDtwTileFloats / F (at most 64) rows in LDS: the wave fetches the next tile into
//                    registers (16 coalesced loads a lane) before it walks the current one, and every lane reads v_t[f] at a uniform
//                    LDS address (a broadcast).  Per step the neighbour's last two (D, n) pairs of the previous column are handed
//                    over by two 64-bit __shfl_up (FPL = 1: from one and from two lanes below), lane 0 takes the free start, and the
//                    lane that owns frame L - 1 leaves (conf, len) of the step in LDS.  After a tile, lane r folds row r into out /
//                    lengths: the keyword's first template stores, a later one replaces what the same lane stored when its conf is
//                    strictly greater -- ascending template order, the first maximum wins.  Two barriers a tile (of a one-wave
//                    workgroup).  RAGGED: the signal's rows are step_off[n] .. step_off[n + 1] - 1; a signal without rows returns at
//                    once.  CARRIED (tcr_dtw_stream_push*): the column before the stream's first row of the call is loaded from the
//                    state (the initial column after a reset) and the one after its last row is stored; a stream without rows is
//                    skipped before either.
//   dtw_bg_kernel    a thread per row: out[t][K] = 1 - max_k out[t][k], behind dtw_kernel (the keywords are different workgroups).
//   dtw_init_kernel  the state of every stream: the detector integers, D = +inf (n = 0 comes from the memset in front of it).
//
// Streaming (tcr_dtw_stream_init / _push / _push_ragged): the scores above and tcr_detect_redetect's detector over them for S live
// streams.  The state: the detector integers [5][S] in scan.hip's layout rounded up to 256 bytes, then D float32 [total_frames x S]
// and n int32 [total_frames x S], template q's block at frame_offsets[q] x S and stream s's L_q values at s x L_q inside it.  A push
// is four launches in stream order: dtw_kernel<.., CARRIED>, dtw_bg_kernel, detect_smooth_kernel at one vector per decision
// (tcr_detect_redetect's own instance) and scan_suppress_kernel (scan.hip) from the carried integers.  A stream without rows in a
// ragged call is skipped by all of them: its state stays byte for byte, its reset flag is ignored.  The last two are the carried
// posterior tail phrase.hip shares (posterior_tail_args, detect_grid.hip, in front of the first launch; suppress_launch, scan.hip); the
// integers' size, initial values and the row checks are scan.hip's (detect_state_ints_bytes, detect_ints_init, detect_*_check).
//
// Limits: F <= TCR_DTW_MAX_FEATURES, Q <= TCR_DTW_MAX_TEMPLATES, L <= tcr_dtw_frames_max(F) = min(256, 4096 / F) (four frames a lane,
// and a wave's template frames within 32 KB of LDS: 256 up to F = 16, 64 at F = 64); there is no path above them.  frame_offsets,
// keyword_offsets and scale travel as kernel arguments (776 bytes), read with uniform indices only.  Nothing is copied and nothing is
// waited for: the entries can be captured into a graph.  Every loop is bounded by the row, frame and template counts.
//
// Known limit: a walk is sequential in t, and the templates of a keyword share a wave, so the parallelism of a call is N x K waves --
// a single long recording with one keyword runs on one wave.  A one-step push stages a template (L x F loads) to take one step.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after stream_cascade.hip).
#pragma once
#include <climits>
#include <cmath>

namespace tcr {

namespace {

constexpr int kDtwMaxTemplates = TCR_DTW_MAX_TEMPLATES;
constexpr int kDtwMaxFeatures = TCR_DTW_MAX_FEATURES;
constexpr int kDtwMaxFpl = 4;                           // frames a lane owns at most
constexpr int kDtwTileFloats = 1024;                    // floats of a staged tile of rows: 16 loads a lane
constexpr int kDtwTileRowsMax = 64;                     // rows of a tile at most: lane r folds row r

// the largest template the kernel takes at F features (< 1: none)
int dtw_frames_max(int F) {
    if (F < 1 || F > kDtwMaxFeatures) return 0;
    const int by_lds = 4096 / F;
    return by_lds < kDtwMaxFpl * kWave ? by_lds : kDtwMaxFpl * kWave;
}

}  // namespace

struct DtwArgs {
    const float* values;        // [N][steps][F] (ragged: packed)
    const float* tmpl;          // [total_frames][F]
    float* out;                 // [..][K + 1]
    int32_t* lengths;           // [..][K] or null
    const int64_t* step_off;    // ragged: [N + 1]
    int64_t steps;              // dense: steps per signal
    int64_t total;              // the call's rows in all
    int N, F, Q, K, max_steps;
    // the carried arm (tcr_dtw_stream_push*): null in the whole-scan entries
    float* st_D;                // [total_frames x N]
    int32_t* st_n;
    const uint8_t* reset;       // [N] or null
    int32_t frame_off[kDtwMaxTemplates + 1];
    int32_t kw_off[kDtwMaxTemplates + 1];
    float scale[kDtwMaxTemplates];
};

__device__ __forceinline__ long long dtw_pack(float d, int n) {
    return (long long)(((unsigned long long)(unsigned)n << 32) | (unsigned long long)__builtin_bit_cast(unsigned, d));
}
__device__ __forceinline__ float dtw_pack_d(long long p) { return __builtin_bit_cast(float, (unsigned)((unsigned long long)p & 0xffffffffull)); }
__device__ __forceinline__ int dtw_pack_n(long long p) { return (int)((unsigned long long)p >> 32); }

// One template over the signal's rows, by the wave: see the file comment.  `first`: the keyword's first template (it stores, the others
// compare).  s_T: the lanes' template frames (dynamic LDS), s_v: a tile of rows, s_conf / s_len: the tile's results.
template <int FPL, bool CARRIED>
__device__ __forceinline__ void dtw_template(const DtwArgs& a, int q, int k, bool first, int sig, int64_t row0, int len, bool fresh, float* s_T,
                                             float* s_v, float* s_conf, int* s_len) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, F = a.F, K = a.K;
    const int f0 = a.frame_off[q], L = a.frame_off[q + 1] - f0;
    const int j0 = lane * FPL;
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
        const bool in = j0 + i < L;
        const float* src = a.tmpl + (size_t)(f0 + (in ? j0 + i : 0)) * F;
        for (int f = 0; f < F; ++f) s_T[(i * F + f) * kWave + lane] = in ? src[f] : 0.f;
    }
    float D[FPL];
    int n[FPL];
    const size_t st_at = (size_t)a.N * f0 + (size_t)sig * L;
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
        const bool load = CARRIED && !fresh && j0 + i < L;
        D[i] = load ? a.st_D[st_at + j0 + i] : INFINITY;
        n[i] = load ? a.st_n[st_at + j0 + i] : 0;
    }
    const int wl = (L - 1) / FPL, wi = (L - 1) - wl * FPL;      // the lane and the register of frame L - 1
    const float scale = a.scale[q];
    const int tile_rows = kDtwTileFloats / F < kDtwTileRowsMax ? kDtwTileFloats / F : kDtwTileRowsMax;
    const float* rows_at = a.values + row0 * F;
    float pre[kDtwTileFloats / kWave];
    auto fetch = [&](int t0) {
        const int cnt = (len - t0 < tile_rows ? len - t0 : tile_rows) * F;
        const float* src = rows_at + (int64_t)t0 * F;
#pragma unroll
        for (int e = 0; e < kDtwTileFloats / kWave; ++e) pre[e] = e * kWave + lane < cnt ? src[e * kWave + lane] : 0.f;
    };
    fetch(0);
    for (int t0 = 0; t0 < len; t0 += tile_rows) {
        const int rows = len - t0 < tile_rows ? len - t0 : tile_rows;
#pragma unroll
        for (int e = 0; e < kDtwTileFloats / kWave; ++e) s_v[e * kWave + lane] = pre[e];
        __syncthreads();                                // (behind the previous tile's fold, which read s_conf / s_len only)
        if (t0 + tile_rows < len) fetch(t0 + tile_rows);
        for (int r = 0; r < rows; ++r) {
            // the previous column: frames j0 - 2, j0 - 1 from the lanes below, then the lane's own
            float oD[FPL + 2];
            int on[FPL + 2];
            const long long p1 = __shfl_up(dtw_pack(D[FPL - 1], n[FPL - 1]), 1);
            const long long p2 = FPL == 1 ? __shfl_up(dtw_pack(D[0], n[0]), 2) : __shfl_up(dtw_pack(D[FPL > 1 ? FPL - 2 : 0], n[FPL > 1 ? FPL - 2 : 0]), 1);
            oD[1] = dtw_pack_d(p1); on[1] = dtw_pack_n(p1);
            oD[0] = dtw_pack_d(p2); on[0] = dtw_pack_n(p2);
            if (lane == 0) {                            // frame 0: the free start on the diagonal, no skip; frame 1 skips from the start
                oD[1] = 0.f; on[1] = 0;
                oD[0] = INFINITY; on[0] = 0;
            } else if (FPL == 1 && lane == 1) {
                oD[0] = 0.f; on[0] = 0;
            }
#pragma unroll
            for (int i = 0; i < FPL; ++i) { oD[i + 2] = D[i]; on[i + 2] = n[i]; }
            float acc[FPL];
#pragma unroll
            for (int i = 0; i < FPL; ++i) acc[i] = 0.f;
            const float* vr = s_v + r * F;
#pragma unroll 4                                        // (four features' LDS reads in flight in front of their dependent adds)
            for (int f = 0; f < F; ++f) {
                const float v = vr[f];
#pragma unroll
                for (int i = 0; i < FPL; ++i) acc[i] = acc[i] + fabsf(s_T[(i * F + f) * kWave + lane] - v);
            }
#pragma unroll
            for (int i = 0; i < FPL; ++i) {
                float bD = oD[i + 1];                   // diag, then stay, then skip: strict comparisons keep the earlier
                int bn = on[i + 1];
                if (oD[i + 2] < bD) { bD = oD[i + 2]; bn = on[i + 2]; }
                if (oD[i] < bD) { bD = oD[i]; bn = on[i]; }
                D[i] = acc[i] + bD;
                n[i] = (bn < INT_MAX - 1 ? bn : INT_MAX - 1) + 1;
            }
            if (lane == wl) {
                float cost = D[0];
                int ln = n[0];
#pragma unroll
                for (int i = 1; i < FPL; ++i)
                    if (i == wi) { cost = D[i]; ln = n[i]; }
                const float prod = cost * scale;
                float c = fmaxf(1.0f - prod, 0.0f);
                if (a.max_steps > 0 && ln > a.max_steps) c = 0.0f;
                s_conf[r] = c;
                s_len[r] = ln;
            }
        }
        __syncthreads();
        if (lane < rows) {
            const int64_t row = row0 + t0 + lane;
            const float c = s_conf[lane];
            float* o = a.out + row * (K + 1) + k;
            if (first || c > *o) {
                *o = c;
                if (a.lengths) a.lengths[row * K + k] = s_len[lane];
            }
        }
    }
    if constexpr (CARRIED) {
#pragma unroll
        for (int i = 0; i < FPL; ++i) {
            if (j0 + i < L) {
                a.st_D[st_at + j0 + i] = D[i];
                a.st_n[st_at + j0 + i] = n[i];
            }
        }
    }
}

// Dynamic LDS: the lanes' template frames [FPL F][64] of the call's longest template; static: a tile of rows and its results.  See
// profiles/dtw_kernel_regs.txt for registers and scratch.
template <bool RAGGED, bool CARRIED>
__global__ __launch_bounds__(64) void dtw_kernel(const DtwArgs a) {
    __shared__ float s_v[kDtwTileFloats];
    __shared__ float s_conf[kDtwTileRowsMax];
    __shared__ int s_len[kDtwTileRowsMax];
    float* s_T = reinterpret_cast<float*>(dyn_lds());
    const int sig = blockIdx.x, k = blockIdx.y;
    const int64_t row0 = RAGGED ? a.step_off[sig] : sig * a.steps;
    const int len = (int)(RAGGED ? a.step_off[sig + 1] - row0 : a.steps);
    if (len <= 0) return;                               // (ragged: a signal without rows; the carried arm: its state stays as it is)
    const bool fresh = !CARRIED || (a.reset && a.reset[sig]);
    for (int q = a.kw_off[k]; q < a.kw_off[k + 1]; ++q) {
        const bool first = q == a.kw_off[k];
        const int L = a.frame_off[q + 1] - a.frame_off[q];
        switch ((L + kWave - 1) / kWave) {              // (uniform)
            case 1: dtw_template<1, CARRIED>(a, q, k, first, sig, row0, len, fresh, s_T, s_v, s_conf, s_len); break;
            case 2: dtw_template<2, CARRIED>(a, q, k, first, sig, row0, len, fresh, s_T, s_v, s_conf, s_len); break;
            case 3: dtw_template<3, CARRIED>(a, q, k, first, sig, row0, len, fresh, s_T, s_v, s_conf, s_len); break;
            default: dtw_template<4, CARRIED>(a, q, k, first, sig, row0, len, fresh, s_T, s_v, s_conf, s_len); break;
        }
    }
}

// the background class, behind dtw_kernel: a thread per row
__global__ __launch_bounds__(256) void dtw_bg_kernel(const DtwArgs a) {
#pragma clang fp contract(off)
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= a.total) return;
    float* o = a.out + row * (a.K + 1);
    float best = o[0];
    for (int k = 1; k < a.K; ++k) best = o[k] > best ? o[k] : best;
    o[a.K] = 1.0f - best;
}

// every stream: no rows seen, no detection yet (head, count, prev_label, prev_step, n), every D +inf (the memset in front left n = 0)
__global__ __launch_bounds__(256) void dtw_init_kernel(int* ist, float* st_D, int S, int64_t n_D) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (!detect_ints_init(ist, S, i) && i - 5 * (int64_t)S < n_D) st_D[i - 5 * (int64_t)S] = INFINITY;
}

namespace {

// The tables and cfg of a call into `a` (frame_off, kw_off, scale, F, Q, K, max_steps, tmpl), with the refusals every entry shares.
int dtw_tables(const char* what, int n_features, int n_templates, const float* templates, const int32_t* frame_offsets, int n_keywords,
               const int32_t* keyword_offsets, const float* scale, const tcr_dtw_cfg* cfg, DtwArgs& a) {
    TCR_REQUIRE(templates && frame_offsets && keyword_offsets && scale && cfg, "%s: null argument", what);
    TCR_REQUIRE(n_features > 0, "%s: n_features must be positive (got %d)", what, n_features);
    TCR_REQUIRE(n_features <= kDtwMaxFeatures, "%s: n_features %d above TCR_DTW_MAX_FEATURES = %d", what, n_features, kDtwMaxFeatures);
    TCR_REQUIRE(n_templates >= 1 && n_templates <= kDtwMaxTemplates, "%s: n_templates %d outside 1..%d", what, n_templates, kDtwMaxTemplates);
    TCR_REQUIRE(n_keywords >= 1 && n_keywords <= n_templates, "%s: n_keywords %d outside 1..%d (the templates)", what, n_keywords, n_templates);
    TCR_REQUIRE(frame_offsets[0] == 0, "%s: frame_offsets must start at 0 (got %d)", what, frame_offsets[0]);
    const int l_max = dtw_frames_max(n_features);
    for (int q = 0; q < n_templates; ++q) {
        const int64_t L = (int64_t)frame_offsets[q + 1] - frame_offsets[q];
        TCR_REQUIRE(L >= 0, "%s: frame_offsets decrease at template %d (%d after %d)", what, q, frame_offsets[q + 1], frame_offsets[q]);
        TCR_REQUIRE(L >= 1 && L <= l_max, "%s: template %d has %lld frames (1..tcr_dtw_frames_max(%d) = %d)", what, q, (long long)L, n_features,
                    l_max);
        TCR_REQUIRE(std::isfinite(scale[q]) && scale[q] > 0.f, "%s: scale[%d] = %g must be finite and > 0", what, q, (double)scale[q]);
    }
    TCR_REQUIRE(keyword_offsets[0] == 0, "%s: keyword_offsets must start at 0 (got %d)", what, keyword_offsets[0]);
    for (int k = 0; k < n_keywords; ++k) {
        const int64_t m = (int64_t)keyword_offsets[k + 1] - keyword_offsets[k];
        TCR_REQUIRE(m >= 0, "%s: keyword_offsets decrease at keyword %d (%d after %d)", what, k, keyword_offsets[k + 1], keyword_offsets[k]);
        TCR_REQUIRE(m >= 1, "%s: keyword %d has no template", what, k);
    }
    TCR_REQUIRE(keyword_offsets[n_keywords] == n_templates, "%s: keyword_offsets must end at n_templates = %d (got %d)", what, n_templates,
                keyword_offsets[n_keywords]);
    TCR_REQUIRE(cfg->max_steps >= 0, "%s: max_steps must be >= 0 (got %d)", what, cfg->max_steps);
    for (int q = 0; q <= n_templates; ++q) a.frame_off[q] = frame_offsets[q];
    for (int k = 0; k <= n_keywords; ++k) a.kw_off[k] = keyword_offsets[k];
    for (int q = 0; q < n_templates; ++q) a.scale[q] = scale[q];
    a.tmpl = templates; a.F = n_features; a.Q = n_templates; a.K = n_keywords; a.max_steps = cfg->max_steps;
    return TCR_OK;
}

// dtw_kernel over the call's (signal, keyword) pairs and the background behind it
template <bool CARRIED>
int dtw_launch(const DtwArgs& a, bool ragged, hipStream_t s) {
    int fpl = 1;
    for (int q = 0; q < a.Q; ++q) fpl = std::max(fpl, ceil_div(a.frame_off[q + 1] - a.frame_off[q], kWave));
    const size_t lds = (size_t)fpl * kWave * a.F * sizeof(float);        // <= 32256 bytes: (4096 / F + 63) F floats
    const auto kernel = ragged ? dtw_kernel<true, CARRIED> : dtw_kernel<false, CARRIED>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)a.N, (unsigned)a.K), dim3(kWave), lds, s, a);
    TCR_TRY(check_launch("dtw_kernel"));
    hipLaunchKernelGGL(dtw_bg_kernel, dim3((unsigned)ceil_div64(a.total, 256)), dim3(256), 0, s, a);
    return check_launch("dtw_bg_kernel");
}

int dtw_scores(const char* what, bool ragged, int n_signals, int64_t steps, const int64_t* step_offsets, int64_t total_steps, int n_features,
               const float* values, int n_templates, const float* templates, const int32_t* frame_offsets, int n_keywords,
               const int32_t* keyword_offsets, const float* scale, const tcr_dtw_cfg* cfg, float* out, int32_t* lengths, void* stream) {
    TCR_REQUIRE((!ragged || step_offsets) && values && out, "%s: null argument", what);
    DtwArgs a{};
    TCR_TRY(dtw_tables(what, n_features, n_templates, templates, frame_offsets, n_keywords, keyword_offsets, scale, cfg, a));
    TCR_TRY(detect_rows_check(what, ragged, n_signals, steps, total_steps, "signals"));
    TCR_TRY(detect_size_check(what, ragged, n_signals, steps, total_steps, n_features, n_keywords + 1));
    a.values = values; a.out = out; a.lengths = lengths; a.step_off = ragged ? step_offsets : nullptr;
    a.steps = steps; a.total = ragged ? total_steps : steps * n_signals; a.N = n_signals;
    return dtw_launch<false>(a, ragged, static_cast<hipStream_t>(stream));
}

// The stream state: | the detector integers [5][S] int32 (scan.hip's layout; at one vector per decision head stays 0 and count 1, and n
// is the rows the stream has seen), detect_state_ints_bytes(S) | D float32 [total_frames x S] | n int32 [total_frames x S] |.

int dtw_stream_geom(const char* what, int n_streams, int n_features, int n_templates, const float* templates, const int32_t* frame_offsets,
                    int n_keywords, const int32_t* keyword_offsets, const float* scale, const tcr_dtw_cfg* cfg, DtwArgs& a) {
    TCR_TRY(dtw_tables(what, n_features, n_templates, templates, frame_offsets, n_keywords, keyword_offsets, scale, cfg, a));
    TCR_REQUIRE(n_streams > 0, "%s: the number of streams must be positive (got %d)", what, n_streams);
    a.N = n_streams;
    return TCR_OK;
}

int dtw_stream_push(const char* what, bool ragged, int n_streams, int64_t steps, const int64_t* step_offsets, int64_t total_steps, int n_features,
                    const float* values, int n_templates, const float* templates, const int32_t* frame_offsets, int n_keywords,
                    const int32_t* keyword_offsets, const float* scale, const tcr_dtw_cfg* cfg, const tcr_detect_cfg* det, const uint8_t* reset,
                    void* state, float* post, int32_t* lengths, int32_t* top, float* score, int32_t* is_new, void* stream) {
    TCR_REQUIRE((!ragged || step_offsets) && values && det && state && post && top && score && is_new, "%s: null argument", what);
    DtwArgs a{};
    TCR_TRY(dtw_stream_geom(what, n_streams, n_features, n_templates, templates, frame_offsets, n_keywords, keyword_offsets, scale, cfg, a));
    TCR_TRY(detect_rows_check(what, ragged, n_streams, steps, total_steps, "streams"));
    ScanDetectArgs da;
    TCR_TRY(posterior_tail_args(what, "template", det, reset, static_cast<int*>(state), post, top, score, is_new, ragged, steps, total_steps,
                                step_offsets, n_streams, n_keywords + 1, da));
    TCR_TRY(detect_size_check(what, ragged, n_streams, steps, total_steps, n_features, n_keywords + 1));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t rows = ragged ? total_steps : steps * n_streams;
    const size_t n_D = (size_t)a.frame_off[a.Q] * n_streams;
    a.values = values; a.out = post; a.lengths = lengths; a.step_off = ragged ? step_offsets : nullptr;
    a.steps = steps; a.total = rows;
    a.st_D = reinterpret_cast<float*>(static_cast<char*>(state) + detect_state_ints_bytes(n_streams));
    a.st_n = reinterpret_cast<int32_t*>(a.st_D + n_D);
    a.reset = reset;
    // 1. the posteriors and lengths, from the carried columns; the columns after the call's rows
    TCR_TRY(dtw_launch<true>(a, ragged, s));
    // 2. top / score and the candidate flags: tcr_detect_redetect's own smoothing instance at one vector per decision
    TCR_TRY(smooth_launch<kSmoothNoVector>(da, ragged, rows, s));
    // 3. the suppression walk from the carried detector, and the integers (n += the stream's rows)
    return suppress_launch(da, ragged, s);
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_dtw_frames_max(int n_features) { return dtw_frames_max(n_features); }

extern "C" int tcr_dtw_scores(int n_signals, int64_t steps, int n_features, const float* values, int n_templates, const float* templates,
                              const int32_t* frame_offsets, int n_keywords, const int32_t* keyword_offsets, const float* scale,
                              const tcr_dtw_cfg* cfg, float* out, int32_t* lengths, void* stream) {
    return dtw_scores("tcr_dtw_scores", false, n_signals, steps, nullptr, 0, n_features, values, n_templates, templates, frame_offsets, n_keywords,
                      keyword_offsets, scale, cfg, out, lengths, stream);
}

extern "C" int tcr_dtw_scores_ragged(int n_signals, const int64_t* step_offsets, int64_t total_steps, int n_features, const float* values,
                                     int n_templates, const float* templates, const int32_t* frame_offsets, int n_keywords,
                                     const int32_t* keyword_offsets, const float* scale, const tcr_dtw_cfg* cfg, float* out, int32_t* lengths,
                                     void* stream) {
    return dtw_scores("tcr_dtw_scores_ragged", true, n_signals, 0, step_offsets, total_steps, n_features, values, n_templates, templates,
                      frame_offsets, n_keywords, keyword_offsets, scale, cfg, out, lengths, stream);
}

extern "C" size_t tcr_dtw_stream_state_bytes(int n_streams, int n_features, int n_templates, const float* templates, const int32_t* frame_offsets,
                                             int n_keywords, const int32_t* keyword_offsets, const float* scale, const tcr_dtw_cfg* cfg) {
    DtwArgs a{};
    if (dtw_stream_geom("tcr_dtw_stream_state_bytes", n_streams, n_features, n_templates, templates, frame_offsets, n_keywords, keyword_offsets,
                        scale, cfg, a) != TCR_OK)
        return 0;
    return detect_state_ints_bytes(n_streams) + (size_t)a.frame_off[a.Q] * n_streams * 8;
}

extern "C" int tcr_dtw_stream_init(int n_streams, int n_features, int n_templates, const float* templates, const int32_t* frame_offsets,
                                   int n_keywords, const int32_t* keyword_offsets, const float* scale, const tcr_dtw_cfg* cfg, void* state,
                                   void* stream) {
    const char* what = "tcr_dtw_stream_init";
    TCR_REQUIRE(state, "%s: null argument", what);
    DtwArgs a{};
    TCR_TRY(dtw_stream_geom(what, n_streams, n_features, n_templates, templates, frame_offsets, n_keywords, keyword_offsets, scale, cfg, a));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t ints = detect_state_ints_bytes(n_streams), n_D = (size_t)a.frame_off[a.Q] * n_streams;
    if (hipMemsetAsync(state, 0, ints + n_D * 8, s) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", what);
        return TCR_ERR_HIP;
    }
    hipLaunchKernelGGL(dtw_init_kernel, dim3((unsigned)ceil_div64((int64_t)5 * n_streams + (int64_t)n_D, 256)), dim3(256), 0, s,
                       static_cast<int*>(state), reinterpret_cast<float*>(static_cast<char*>(state) + ints), n_streams, (int64_t)n_D);
    return check_launch("dtw_init_kernel");
}

extern "C" int tcr_dtw_stream_push(int n_streams, int64_t steps, int n_features, const float* values, int n_templates, const float* templates,
                                   const int32_t* frame_offsets, int n_keywords, const int32_t* keyword_offsets, const float* scale,
                                   const tcr_dtw_cfg* cfg, const tcr_detect_cfg* det, const uint8_t* reset, void* state, float* post,
                                   int32_t* lengths, int32_t* top, float* score, int32_t* is_new, void* stream) {
    return dtw_stream_push("tcr_dtw_stream_push", false, n_streams, steps, nullptr, 0, n_features, values, n_templates, templates, frame_offsets,
                           n_keywords, keyword_offsets, scale, cfg, det, reset, state, post, lengths, top, score, is_new, stream);
}

extern "C" int tcr_dtw_stream_push_ragged(int n_streams, const int64_t* step_offsets, int64_t total_steps, int n_features, const float* values,
                                          int n_templates, const float* templates, const int32_t* frame_offsets, int n_keywords,
                                          const int32_t* keyword_offsets, const float* scale, const tcr_dtw_cfg* cfg, const tcr_detect_cfg* det,
                                          const uint8_t* reset, void* state, float* post, int32_t* lengths, int32_t* top, float* score,
                                          int32_t* is_new, void* stream) {
    return dtw_stream_push("tcr_dtw_stream_push_ragged", true, n_streams, 0, step_offsets, total_steps, n_features, values, n_templates, templates,
                           frame_offsets, n_keywords, keyword_offsets, scale, cfg, det, reset, state, post, lengths, top, score, is_new, stream);
}
