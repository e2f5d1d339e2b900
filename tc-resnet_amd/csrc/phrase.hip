// Phrase scores from a scan's posteriors (tcr_phrase_scores, tcr_phrase_scores_ragged): values [steps][C] word posteriors in, out
// [steps][P + 1] phrase posteriors -- per phrase the best fold (product or min) of its words' values over a sliding window of w steps,
// the words in order (ordered) or each at its own maximum (unordered), and the background 1 - max over the phrases last -- so that
// the detector, sweep, grid and mining entries apply to phrases with num_classes = P + 1.  The contract (include/tcresnet_hip.h) fixes
// the float32 operations and their order; the kernel evaluates exactly those.
//
//   phrase_kernel             a workgroup per tile of TCR_PHRASE_TILE consecutive steps of one signal.  It stages the tile's rows and
//                             the h = min(w - 1, first step of the tile) rows in front of them (rows before the signal's first step
//                             are never read), but only the U distinct word classes of the phrases, planar: column u at
//                             s_p[u * (TILE + w - 1) + row].  Then a lane per step: for every phrase the DP state E[n] lives in
//                             registers (the word count is uniform: one fully unrolled instance per count 1 .. 8, ordered / unordered
//                             and product / min, chosen by a uniform switch; no scratch) and walks the step's count = min(i + 1, w)
//                             rows oldest first,
//                                 ordered:    E[0] = max(E[0], v[t][c_1]),  E[m] = max(E[m], f(E[m - 1], v[t][c_m + 1])), m ascending,
//                                 unordered:  E[m] = max(E[m], v[t][c_m + 1]), folded left to right at the end,
//                             from -inf (every E[m - 1] read was written in the same row, so the start value is never an operand of
//                             f).  Consecutive lanes walk consecutive steps, so every LDS read of a wave is 64 consecutive floats of one
//                             column: no bank conflict whatever C and w (row-major [step][C] would be a 4-way conflict at C = 12).
//                             The lane writes its step's P + 1 outputs with plain stores.
//   Ragged tiles without a host copy of the offsets: detect_grid.hip's scheme -- signal n's tiles are blocks f(n) .. with f(n) =
//   step_off[n] / TILE + n, floor(total / TILE) + N blocks cover every tile, a block finds its signal by binary search over f and
//   returns when its tile lies past the signal's last step.
//
// Streaming (tcr_phrase_stream_init / _push / _push_ragged): the same posteriors and tcr_detect_redetect's detector over them for S live
// streams, with the last w - 1 rows of every stream (staged columns only) and the detector integers carried in a caller-owned state,
// so that any split of a stream into pushes gives the whole scan's bits.  The state: the integers [5][S] in scan.hip's layout, then a
// ring [w - 1][U][S] in which row r of a stream (counted from its reset) lies in slot r mod (w - 1) -- no head is stored, and streams
// that advance by different amounts simply stand at different slots.  A push is four launches in stream order:
//   1. the posteriors, from the old ring and row counts: phrase_lane_kernel when the call brings at most kPhraseLaneRows rows a
//      stream on average (a server's one-step pushes: a lane per row, phrases dealt to the waves, the window walked in global
//      memory, where consecutive lanes are consecutive streams of the planar ring), else phrase_kernel<.., CARRIED> (a recording
//      in chunks: the rows in front of a stream's first tile staged from the ring);
//   2. detect_smooth_kernel at one vector per decision (tcr_detect_redetect's own instance): top, score, candidate flags;
//   3. phrase_hist_kernel: the call's last min(m_s, w - 1) rows into their ring slots -- behind every reader of the old rows, and
//      before the row counts move;
//   4. scan_suppress_kernel (scan.hip) from the carried integers: is_new, and the integers (n += m_s).
//   A stream without rows in a ragged call is skipped by all four: its state stays byte for byte, its reset flag is ignored.
//   2 and 4 are the carried posterior tail dtw.hip shares (posterior_tail_args, detect_grid.hip, in front of launch 1; suppress_launch,
//   scan.hip); the integers' size, initial values and the row checks are scan.hip's (detect_state_ints_bytes, detect_ints_init, detect_*_check).
//
// The LDS limit: (TCR_PHRASE_TILE + w - 1) x U floats of dynamic LDS within 64 KB a workgroup (no static LDS next to it), i.e.
// tcr_phrase_window_max(U) = 16384 / U - 255 (U = 4: 3841, U = 12: 1110, U = 64: 1; none above).  There is no path above it.
// The phrase tables travel as kernel arguments (64 word counts, 64 staged classes, 64 x 8 staged-column indices: 832 bytes), read with
// uniform indices only.  Nothing is copied and nothing is waited for: the entries can be captured into a graph.
//
// The walk costs w x n LDS reads per (step, phrase of n words); at the window sizes in use (75 - 150 steps) a prefix / suffix scheme
// would cut that for `min` only -- the product does not re-associate bitwise -- and is not built.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after mine.hip).
#pragma once
#include <cmath>

namespace tcr {

namespace {

constexpr int kPhraseTile = TCR_PHRASE_TILE;
constexpr int kPhraseMaxWords = TCR_PHRASE_MAX_WORDS;
constexpr int kPhraseMax = TCR_PHRASE_MAX;
constexpr int kPhraseMaxCols = 64;                      // distinct word classes a call can stage (window_max(64) = 1)
constexpr int kPhraseLdsFloats = 64 * 1024 / 4;         // dynamic LDS floats of phrase_kernel

// the largest window the staged kernel takes with U distinct word classes (< 1: none)
int phrase_w_max(int U) { return U >= 1 ? kPhraseLdsFloats / U - (kPhraseTile - 1) : 0; }

}  // namespace

struct PhraseArgs {
    const float* values;        // [N][steps][C] (ragged: packed)
    float* out;                 // [..][P + 1]
    const int64_t* step_off;    // ragged: [N + 1]
    int64_t steps, tiles;       // dense: steps and tiles per signal
    int N, C, P, U, w, stride;  // stride = TILE + w - 1: floats between two staged columns
    int ordered, combine;
    // the carried arm (tcr_phrase_stream_push*): the stream state, null / 0 in the whole-scan entries
    float* ring;                // [H][U][N]: row r of stream s (counted from its reset) is in slot r % H
    int* ist;                   // [5][N]: the detector integers of scan.hip; ist[4 N + s] = the rows stream s has seen
    const uint8_t* reset;       // [N] or null
    int H;                      // w - 1 ring slots
    int64_t total;              // the call's rows in all
    uint8_t n_words[kPhraseMax];
    int32_t col_class[kPhraseMaxCols];                  // staged column u holds class col_class[u]
    uint8_t word_col[kPhraseMax][kPhraseMaxWords];      // the staged column of phrase q's word m
};

template <bool MIN>
__device__ __forceinline__ float phrase_f(float x, float y) {
    return MIN ? fminf(x, y) : x * y;
}

// conf of one phrase of NW words at one step: s_at is the step's oldest row in column 0, ofs[m] the float offset of word m's column.
template <int NW, bool ORDERED, bool MIN>
__device__ __forceinline__ float phrase_conf(const float* s_at, int count, const int (&ofs)[kPhraseMaxWords]) {
    float E[NW];
#pragma unroll
    for (int m = 0; m < NW; ++m) E[m] = -INFINITY;
    for (int k = 0; k < count; ++k) {
#pragma unroll
        for (int m = 0; m < NW; ++m) {
            const float v = s_at[ofs[m] + k];
            if (ORDERED && m > 0) E[m] = fmaxf(E[m], phrase_f<MIN>(E[m - 1], v));
            else E[m] = fmaxf(E[m], v);
        }
    }
    if (ORDERED) return E[NW - 1];
    float r = E[0];
#pragma unroll
    for (int m = 1; m < NW; ++m) r = phrase_f<MIN>(r, E[m]);
    return r;
}

// The same walk over rows that are not staged (phrase_lane_kernel): the step's window as three runs of rows in global memory -- the
// ring up to its last slot, the ring from slot 0, the call's own rows -- word m's value in run j's k-th row at
// at[j][ofs[j == 2][m] + k * stride[j]].  The DP state goes through the runs in turn: the same operations on the same rows, oldest
// first.  (The staged form above stays as it was written, its arguments by value: behind a row getter shared with this one its ordered
// instances ran 2 - 4 % slower on the MI355X -- 46 / 50 VGPRs instead of 58 / 62, another unrolling.)
struct PhraseRuns {
    const float* at[3];
    int count[3];
    size_t stride[3];
};

template <int NW, bool ORDERED, bool MIN>
__device__ __forceinline__ float phrase_conf(const PhraseRuns& r, const int (&ofs)[2][kPhraseMaxWords]) {
    float E[NW];
#pragma unroll
    for (int m = 0; m < NW; ++m) E[m] = -INFINITY;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float* at = r.at[j];
        const size_t stride = r.stride[j];
        for (int k = 0; k < r.count[j]; ++k) {
#pragma unroll
            for (int m = 0; m < NW; ++m) {
                const float v = at[ofs[j == 2][m] + k * stride];
                if (ORDERED && m > 0) E[m] = fmaxf(E[m], phrase_f<MIN>(E[m - 1], v));
                else E[m] = fmaxf(E[m], v);
            }
        }
    }
    if (ORDERED) return E[NW - 1];
    float c = E[0];
#pragma unroll
    for (int m = 1; m < NW; ++m) c = phrase_f<MIN>(c, E[m]);
    return c;
}

// one fully unrolled instance per word count, chosen by a uniform switch: the staged rows, and the runs
template <bool ORDERED, bool MIN>
__device__ __forceinline__ float phrase_conf_n(int nw, const float* s_at, int count, const int (&ofs)[kPhraseMaxWords]) {
    switch (nw) {                                       // (uniform)
        case 1: return phrase_conf<1, ORDERED, MIN>(s_at, count, ofs);
        case 2: return phrase_conf<2, ORDERED, MIN>(s_at, count, ofs);
        case 3: return phrase_conf<3, ORDERED, MIN>(s_at, count, ofs);
        case 4: return phrase_conf<4, ORDERED, MIN>(s_at, count, ofs);
        case 5: return phrase_conf<5, ORDERED, MIN>(s_at, count, ofs);
        case 6: return phrase_conf<6, ORDERED, MIN>(s_at, count, ofs);
        case 7: return phrase_conf<7, ORDERED, MIN>(s_at, count, ofs);
        default: return phrase_conf<8, ORDERED, MIN>(s_at, count, ofs);
    }
}

template <bool ORDERED, bool MIN>
__device__ __forceinline__ float phrase_conf_n(int nw, const PhraseRuns& r, const int (&ofs)[2][kPhraseMaxWords]) {
    switch (nw) {                                       // (uniform)
        case 1: return phrase_conf<1, ORDERED, MIN>(r, ofs);
        case 2: return phrase_conf<2, ORDERED, MIN>(r, ofs);
        case 3: return phrase_conf<3, ORDERED, MIN>(r, ofs);
        case 4: return phrase_conf<4, ORDERED, MIN>(r, ofs);
        case 5: return phrase_conf<5, ORDERED, MIN>(r, ofs);
        case 6: return phrase_conf<6, ORDERED, MIN>(r, ofs);
        case 7: return phrase_conf<7, ORDERED, MIN>(r, ofs);
        default: return phrase_conf<8, ORDERED, MIN>(r, ofs);
    }
}

// the rows stream s has seen before this call (the carried arm): none after a reset
__device__ __forceinline__ int phrase_seen(const PhraseArgs& a, int s) { return a.reset && a.reset[s] ? 0 : a.ist[4 * a.N + s]; }

// Dynamic LDS: the staged columns [U][TILE + w - 1].  No static LDS; see profiles/phrase_kernel_regs.txt for registers and scratch.
// CARRIED (tcr_phrase_stream_push*, the chunk shape): the signal is a stream that has seen n0 rows before the call's, so the rows in
// front of a tile are the last min(w - 1, n0 + i0) of the stream: those of this call from `values`, the older ones from the ring.
template <bool RAGGED, bool CARRIED = false>
__global__ __launch_bounds__(256) void phrase_kernel(const PhraseArgs a) {
    float* s_p = reinterpret_cast<float*>(dyn_lds());
    const int tid = threadIdx.x, C = a.C, P = a.P;
    int64_t row0, i0, len_sig;
    int sig;
    if constexpr (RAGGED) {
        const int64_t b = blockIdx.x;
        int lo = 0, hi = a.N - 1;                       // the last n with step_off[n] / TILE + n <= b
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.step_off[mid] / kPhraseTile + mid <= b) lo = mid;
            else hi = mid - 1;
        }
        sig = lo;
        row0 = a.step_off[lo];
        len_sig = a.step_off[lo + 1] - row0;
        i0 = (b - (row0 / kPhraseTile + lo)) * kPhraseTile;
    } else {
        const int64_t n = blockIdx.x / (uint64_t)a.tiles;
        sig = (int)n;
        row0 = n * a.steps;
        len_sig = a.steps;
        i0 = (blockIdx.x - n * a.tiles) * kPhraseTile;
    }
    if (i0 >= len_sig) return;                          // (ragged: a signal without steps, or a spare block)
    const int len = (int)(len_sig - i0 < kPhraseTile ? len_sig - i0 : kPhraseTile);
    int64_t seen = i0;                                  // the signal's rows in front of the tile
    if constexpr (CARRIED) seen += phrase_seen(a, sig);
    const int h = (int)(seen < a.w - 1 ? seen : a.w - 1);       // those of them the tile's steps read (never before the signal's first)
    const int hr = CARRIED && i0 < h ? h - (int)i0 : 0;         // of them, the rows before this call: from the ring
    const float* src = a.values + (row0 + i0 - (h - hr)) * C;
    const int n_rows = h + len;                         // <= stride
    for (int u = 0; u < a.U; ++u) {
        const int cls = a.col_class[u];
        float* dst = s_p + u * a.stride;
        for (int s = tid; s < n_rows; s += 256) {
            if (CARRIED && s < hr) dst[s] = a.ring[((size_t)((seen - h + s) % a.H) * a.U + u) * a.N + sig];
            else dst[s] = src[(int64_t)(s - hr) * C + cls];
        }
    }
    __syncthreads();
    if (tid >= len) return;                             // (after the kernel's only barrier)
    const int64_t i = seen + tid;
    const int count = i + 1 < a.w ? (int)(i + 1) : a.w;
    const float* s_at = s_p + (h + tid - count + 1);    // >= s_p: count = i + 1 while h = seen, else h = w - 1 = count - 1
    float* o = a.out + (row0 + i0 + tid) * (P + 1);
    float best = 0.f;
    for (int q = 0; q < P; ++q) {
        const int nw = a.n_words[q];
        int ofs[kPhraseMaxWords];
#pragma unroll
        for (int m = 0; m < kPhraseMaxWords; ++m) ofs[m] = a.word_col[q][m] * a.stride;
        float c;
        if (a.ordered) c = a.combine == TCR_PHRASE_MIN ? phrase_conf_n<true, true>(nw, s_at, count, ofs) : phrase_conf_n<true, false>(nw, s_at, count, ofs);
        else c = a.combine == TCR_PHRASE_MIN ? phrase_conf_n<false, true>(nw, s_at, count, ofs) : phrase_conf_n<false, false>(nw, s_at, count, ofs);
        o[q] = c;
        best = q ? fmaxf(best, c) : c;
    }
    o[P] = 1.0f - best;
}

// The carried arm's server shape (many streams, a few rows each in a call): a lane per packed row of the call, 64 rows a workgroup,
// and the phrases dealt to its four waves (phrase q to wave q % 4, so the word count stays uniform in a wave).  Nothing is staged: a
// lane walks its step's count = min(n0 + j + 1, w) rows oldest first, the rows before the call from the stream's ring slots, the
// call's own from `values`.  The ring is planar over the streams -- slot, column, stream -- so where consecutive lanes are
// consecutive streams at the same row count (a dense one-step push) every load of a wave is 64 consecutive floats; streams whose
// counts differ (ragged pushes) read their own slots.  The phrase scores go out with plain stores and to LDS ([P][64] floats,
// dynamic), from where wave 0 folds the background in phrase order after the kernel's only barrier.
template <bool RAGGED>
__global__ __launch_bounds__(256) void phrase_lane_kernel(const PhraseArgs a) {
    float* s_c = reinterpret_cast<float*>(dyn_lds());
    const int lane = threadIdx.x & 63, C = a.C, P = a.P;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;  // the packed row
    const bool live = t < a.total;
    const size_t slot_stride = (size_t)a.U * a.N;
    PhraseRuns runs{};                                  // (a lane past the call's rows: three runs of no rows)
    if (live) {
        int sig;
        int64_t row0;
        if constexpr (RAGGED) {
            sig = ragged_signal(a.step_off, a.N, t);
            row0 = a.step_off[sig];
        } else {
            sig = (int)(t / a.steps);
            row0 = sig * a.steps;
        }
        const int64_t j = t - row0, r = j + phrase_seen(a, sig);       // the row in the call, and in the stream
        const int count = r + 1 < a.w ? (int)(r + 1) : a.w;
        const int nh = j < count - 1 ? count - 1 - (int)j : 0;          // the step's rows before the call: ring slots slot0 .., wrapping
        const int slot0 = nh ? (int)((r - count + 1) % a.H) : 0;
        runs.count[0] = nh < a.H - slot0 ? nh : a.H - slot0;
        runs.count[1] = nh - runs.count[0];
        runs.count[2] = count - nh;
        runs.at[0] = a.ring + slot0 * slot_stride + sig;
        runs.at[1] = a.ring + sig;
        runs.at[2] = a.values + (t - (count - 1 - nh)) * C;            // the step's first row of this call
        runs.stride[0] = runs.stride[1] = slot_stride;
        runs.stride[2] = C;
    }
    for (int q = wave; q < P; q += 4) {
        const int nw = a.n_words[q];
        int ofs[2][kPhraseMaxWords];                    // the ring's columns, the classes of the call's rows
#pragma unroll
        for (int m = 0; m < kPhraseMaxWords; ++m) {
            ofs[0][m] = a.word_col[q][m] * a.N;
            ofs[1][m] = a.col_class[a.word_col[q][m]];
        }
        float c;
        if (a.ordered) c = a.combine == TCR_PHRASE_MIN ? phrase_conf_n<true, true>(nw, runs, ofs) : phrase_conf_n<true, false>(nw, runs, ofs);
        else c = a.combine == TCR_PHRASE_MIN ? phrase_conf_n<false, true>(nw, runs, ofs) : phrase_conf_n<false, false>(nw, runs, ofs);
        if (live) a.out[t * (P + 1) + q] = c;
        s_c[q * 64 + lane] = c;
    }
    __syncthreads();
    if (wave != 0 || !live) return;
    float best = s_c[lane];
    for (int q = 1; q < P; ++q) best = fmaxf(best, s_c[q * 64 + lane]);
    a.out[t * (P + 1) + P] = 1.0f - best;
}

// The ring write-back, launched behind every reader of the old rows: the last min(m_s, H) rows of stream s in this call go to the
// slots of their row numbers, the staged columns only.  A thread per (stream, column, 16 rows); a stream without rows writes nothing.
constexpr int kPhraseHistRows = 16;
template <bool RAGGED>
__global__ __launch_bounds__(256) void phrase_hist_kernel(const PhraseArgs a) {
    const int s = blockIdx.x * 256 + threadIdx.x, u = blockIdx.y;
    if (s >= a.N) return;
    const int64_t row0 = RAGGED ? a.step_off[s] : s * a.steps;
    const int64_t m = RAGGED ? a.step_off[s + 1] - row0 : a.steps;
    const int keep = (int)(m < a.H ? m : a.H);
    const int d0 = blockIdx.z * kPhraseHistRows, d1 = d0 + kPhraseHistRows < keep ? d0 + kPhraseHistRows : keep;
    if (d0 >= d1) return;
    const int64_t first = m - keep, r0 = first + phrase_seen(a, s);     // the first kept row in the call, and in the stream
    const float* src = a.values + (row0 + first) * a.C + a.col_class[u];
    for (int d = d0; d < d1; ++d) a.ring[((size_t)((r0 + d) % a.H) * a.U + u) * a.N + s] = src[(int64_t)d * a.C];
}

// every stream: no rows seen, no detection yet (head, count, prev_label, prev_step, n)
__global__ __launch_bounds__(256) void phrase_init_kernel(int* ist, int S) {
    detect_ints_init(ist, S, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

namespace {

// The phrase tables and cfg of a call into `a` (n_words, col_class, word_col, P, U, w, stride, ordered, combine), with the refusals
// every phrase entry shares.
int phrase_tables(const char* what, int num_classes, int n_phrases, const int32_t* phrase_offsets, const int32_t* phrase_words,
                  const tcr_phrase_cfg* cfg, PhraseArgs& a) {
    TCR_REQUIRE(num_classes > 0, "%s: num_classes must be positive (got %d)", what, num_classes);
    TCR_REQUIRE(n_phrases >= 1 && n_phrases <= kPhraseMax, "%s: n_phrases %d outside 1..%d", what, n_phrases, kPhraseMax);
    TCR_REQUIRE(phrase_offsets[0] == 0, "%s: phrase_offsets must start at 0 (got %d)", what, phrase_offsets[0]);
    int U = 0;
    bool cols_fit = true;
    for (int q = 0; q < n_phrases; ++q) {
        const int first = phrase_offsets[q], n = phrase_offsets[q + 1] - first;
        TCR_REQUIRE(n >= 0, "%s: phrase_offsets decrease at phrase %d (%d after %d)", what, q, phrase_offsets[q + 1], first);
        TCR_REQUIRE(n >= 1 && n <= kPhraseMaxWords, "%s: phrase %d has %d words (1..%d)", what, q, n, kPhraseMaxWords);
        a.n_words[q] = (uint8_t)n;
        for (int m = 0; m < n; ++m) {
            const int c = phrase_words[first + m];
            TCR_REQUIRE(c >= 0 && c < num_classes, "%s: phrase %d word %d: class %d outside 0..%d", what, q, m, c, num_classes - 1);
            const int staged = U < kPhraseMaxCols ? U : kPhraseMaxCols;
            int u = 0;
            while (u < staged && a.col_class[u] != c) ++u;
            if (u == staged) {                          // a new distinct class
                if (U < kPhraseMaxCols) a.col_class[U] = c;
                else {                                  // (more than can be staged at any window: counted on for the message, refused below)
                    cols_fit = false;
                    u = 0;
                }
                ++U;
            }
            a.word_col[q][m] = (uint8_t)u;
        }
    }
    TCR_REQUIRE(cfg->window_steps >= 1, "%s: window_steps must be >= 1 (got %d)", what, cfg->window_steps);
    const int w_max = phrase_w_max(U);
    TCR_REQUIRE(cols_fit && cfg->window_steps <= w_max, "%s: window_steps %d above tcr_phrase_window_max(%d distinct word classes) = %d", what,
                cfg->window_steps, U, w_max);
    TCR_REQUIRE(cfg->ordered == 0 || cfg->ordered == 1, "%s: ordered must be 0 or 1 (got %d)", what, cfg->ordered);
    TCR_REQUIRE(cfg->combine == TCR_PHRASE_PRODUCT || cfg->combine == TCR_PHRASE_MIN, "%s: unknown combine %d (TCR_PHRASE_PRODUCT, TCR_PHRASE_MIN)",
                what, cfg->combine);
    a.C = num_classes; a.P = n_phrases; a.U = U; a.w = cfg->window_steps; a.stride = kPhraseTile + cfg->window_steps - 1;
    a.ordered = cfg->ordered; a.combine = cfg->combine;
    return TCR_OK;
}

// phrase_kernel over the call's tiles: CARRIED from the stream state in `a`
template <bool CARRIED>
int phrase_tile_launch(const char* what, const PhraseArgs& a, bool ragged, int64_t total_steps, hipStream_t s) {
    const int64_t blocks = ragged ? total_steps / kPhraseTile + a.N : a.tiles * a.N;
    const size_t lds = (size_t)a.stride * a.U * sizeof(float);
    const auto kernel = ragged ? phrase_kernel<true, CARRIED> : phrase_kernel<false, CARRIED>;
    if (lds > 32 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
                               hipSuccess) {
        set_error("%s: hipFuncSetAttribute failed", what);
        return TCR_ERR_HIP;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, s, a);
    return check_launch("phrase_kernel");
}

int phrase_scores(const char* what, bool ragged, int n_signals, int64_t steps, const int64_t* step_offsets, int64_t total_steps, int num_classes,
                  const float* values, int n_phrases, const int32_t* phrase_offsets, const int32_t* phrase_words, const tcr_phrase_cfg* cfg,
                  float* out, void* stream) {
    TCR_REQUIRE((!ragged || step_offsets) && values && phrase_offsets && phrase_words && cfg && out, "%s: null argument", what);
    TCR_TRY(detect_rows_check(what, ragged, n_signals, steps, total_steps, "signals"));
    PhraseArgs a{};
    TCR_TRY(phrase_tables(what, num_classes, n_phrases, phrase_offsets, phrase_words, cfg, a));
    TCR_TRY(detect_size_check(what, ragged, n_signals, steps, total_steps, num_classes, n_phrases + 1));
    a.values = values; a.out = out; a.step_off = ragged ? step_offsets : nullptr;
    a.steps = steps; a.tiles = ragged ? 0 : ceil_div64(steps, kPhraseTile);
    a.N = n_signals;
    return phrase_tile_launch<false>(what, a, ragged, total_steps, static_cast<hipStream_t>(stream));
}

// The stream state: | the detector integers [5][S] int32 (scan.hip's layout: head, count, prev_label, prev_step, n; at average_steps = 1
// head stays 0 and count 1, and n doubles as the rows the stream has seen), detect_state_ints_bytes(S) | ring [w - 1][U][S] float32 |.

// what tcr_phrase_stream_state_bytes / _init / _push* check about (S, C, tables, cfg); fills a's tables, N and H
int phrase_stream_geom(const char* what, int n_streams, int num_classes, int n_phrases, const int32_t* phrase_offsets, const int32_t* phrase_words,
                       const tcr_phrase_cfg* cfg, PhraseArgs& a) {
    TCR_TRY(phrase_tables(what, num_classes, n_phrases, phrase_offsets, phrase_words, cfg, a));
    a.N = n_streams;
    a.H = a.w - 1;
    return TCR_OK;
}

// Rows a stream brings on average up to which a push runs the lane kernel (each row walks its window from global memory); above,
// the tile kernel stages every window once for 256 steps.
constexpr int kPhraseLaneRows = 4;

int phrase_stream_push(const char* what, bool ragged, int n_streams, int64_t steps, const int64_t* step_offsets, int64_t total_steps,
                       int num_classes, const float* values, int n_phrases, const int32_t* phrase_offsets, const int32_t* phrase_words,
                       const tcr_phrase_cfg* cfg, const tcr_detect_cfg* det, const uint8_t* reset, void* state, float* post, int32_t* top,
                       float* score, int32_t* is_new, void* stream) {
    TCR_REQUIRE((!ragged || step_offsets) && values && phrase_offsets && phrase_words && cfg && det && state && post && top && score && is_new,
                "%s: null argument", what);
    TCR_TRY(detect_rows_check(what, ragged, n_streams, steps, total_steps, "streams"));
    PhraseArgs a{};
    TCR_TRY(phrase_stream_geom(what, n_streams, num_classes, n_phrases, phrase_offsets, phrase_words, cfg, a));
    ScanDetectArgs da;
    TCR_TRY(posterior_tail_args(what, "phrase", det, reset, static_cast<int*>(state), post, top, score, is_new, ragged, steps, total_steps,
                                step_offsets, n_streams, n_phrases + 1, da));
    TCR_TRY(detect_size_check(what, ragged, n_streams, steps, total_steps, num_classes, n_phrases + 1));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t rows = ragged ? total_steps : steps * n_streams;
    a.values = values; a.out = post; a.step_off = ragged ? step_offsets : nullptr;
    a.steps = steps; a.tiles = ragged ? 0 : ceil_div64(steps, kPhraseTile);
    a.total = rows;
    a.ist = da.st.ist;
    a.ring = reinterpret_cast<float*>(static_cast<char*>(state) + detect_state_ints_bytes(n_streams));
    a.reset = reset;
    // 1. the posteriors, from the old ring and the old row counts
    if (rows <= (int64_t)kPhraseLaneRows * n_streams) {
        const auto lane = ragged ? phrase_lane_kernel<true> : phrase_lane_kernel<false>;
        hipLaunchKernelGGL(lane, dim3((unsigned)ceil_div64(rows, 64)), dim3(256), (size_t)a.P * 64 * sizeof(float), s, a);
        TCR_TRY(check_launch("phrase_lane_kernel"));
    } else {
        TCR_TRY(phrase_tile_launch<true>(what, a, ragged, total_steps, s));
    }
    // 2. top / score and the candidate flags: tcr_detect_redetect's own smoothing instance at one vector per decision
    TCR_TRY(smooth_launch<kSmoothNoVector>(da, ragged, rows, s));
    // 3. the new rows into the ring, behind their readers and before the row counts move
    if (a.H > 0) {
        const int64_t most = ragged ? total_steps : steps;      // (no stream brings more rows)
        const int keep = (int)(most < a.H ? most : a.H);
        const auto hist = ragged ? phrase_hist_kernel<true> : phrase_hist_kernel<false>;
        hipLaunchKernelGGL(hist, dim3((unsigned)ceil_div64(n_streams, 256), a.U, (unsigned)ceil_div64(keep, kPhraseHistRows)), dim3(256), 0, s, a);
        TCR_TRY(check_launch("phrase_hist_kernel"));
    }
    // 4. the suppression walk from the carried detector, and the integers (n += the stream's rows)
    return suppress_launch(da, ragged, s);
}

}  // namespace

}  // namespace tcr

using namespace tcr;

extern "C" int tcr_phrase_window_max(int n_distinct_classes) { return phrase_w_max(n_distinct_classes); }

extern "C" int tcr_phrase_scores(int n_signals, int64_t steps, int num_classes, const float* values, int n_phrases, const int32_t* phrase_offsets,
                                 const int32_t* phrase_words, const tcr_phrase_cfg* cfg, float* out, void* stream) {
    return phrase_scores("tcr_phrase_scores", false, n_signals, steps, nullptr, 0, num_classes, values, n_phrases, phrase_offsets, phrase_words,
                         cfg, out, stream);
}

extern "C" int tcr_phrase_scores_ragged(int n_signals, const int64_t* step_offsets, int64_t total_steps, int num_classes, const float* values,
                                        int n_phrases, const int32_t* phrase_offsets, const int32_t* phrase_words, const tcr_phrase_cfg* cfg,
                                        float* out, void* stream) {
    return phrase_scores("tcr_phrase_scores_ragged", true, n_signals, 0, step_offsets, total_steps, num_classes, values, n_phrases,
                         phrase_offsets, phrase_words, cfg, out, stream);
}

extern "C" size_t tcr_phrase_stream_state_bytes(int n_streams, int num_classes, int n_phrases, const int32_t* phrase_offsets,
                                                const int32_t* phrase_words, const tcr_phrase_cfg* cfg) {
    const char* what = "tcr_phrase_stream_state_bytes";
    PhraseArgs a{};
    if (!(phrase_offsets && phrase_words && cfg)) {
        set_error("%s: null argument", what);
        return 0;
    }
    if (n_streams <= 0) {
        set_error("%s: the number of streams must be positive (got %d)", what, n_streams);
        return 0;
    }
    if (phrase_stream_geom(what, n_streams, num_classes, n_phrases, phrase_offsets, phrase_words, cfg, a) != TCR_OK) return 0;
    return detect_state_ints_bytes(n_streams) + (size_t)a.H * a.U * n_streams * sizeof(float);
}

extern "C" int tcr_phrase_stream_init(int n_streams, int num_classes, int n_phrases, const int32_t* phrase_offsets, const int32_t* phrase_words,
                                      const tcr_phrase_cfg* cfg, void* state, void* stream) {
    const char* what = "tcr_phrase_stream_init";
    TCR_REQUIRE(phrase_offsets && phrase_words && cfg && state, "%s: null argument", what);
    TCR_REQUIRE(n_streams > 0, "%s: the number of streams must be positive (got %d)", what, n_streams);
    PhraseArgs a{};
    TCR_TRY(phrase_stream_geom(what, n_streams, num_classes, n_phrases, phrase_offsets, phrase_words, cfg, a));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t ints = detect_state_ints_bytes(n_streams), ring = (size_t)a.H * a.U * n_streams * sizeof(float);
    if (hipMemsetAsync(state, 0, ints + ring, s) != hipSuccess) {      // (the ring's slots are written before they are read; zeros keep the state's bytes defined)
        set_error("%s: hipMemsetAsync failed", what);
        return TCR_ERR_HIP;
    }
    hipLaunchKernelGGL(phrase_init_kernel, dim3((unsigned)ceil_div64((int64_t)5 * n_streams, 256)), dim3(256), 0, s, static_cast<int*>(state),
                       n_streams);
    return check_launch("phrase_init_kernel");
}

extern "C" int tcr_phrase_stream_push(int n_streams, int64_t steps, int num_classes, const float* values, int n_phrases,
                                      const int32_t* phrase_offsets, const int32_t* phrase_words, const tcr_phrase_cfg* cfg,
                                      const tcr_detect_cfg* det, const uint8_t* reset, void* state, float* post, int32_t* top, float* score,
                                      int32_t* is_new, void* stream) {
    return phrase_stream_push("tcr_phrase_stream_push", false, n_streams, steps, nullptr, 0, num_classes, values, n_phrases, phrase_offsets,
                              phrase_words, cfg, det, reset, state, post, top, score, is_new, stream);
}

extern "C" int tcr_phrase_stream_push_ragged(int n_streams, const int64_t* step_offsets, int64_t total_steps, int num_classes, const float* values,
                                             int n_phrases, const int32_t* phrase_offsets, const int32_t* phrase_words, const tcr_phrase_cfg* cfg,
                                             const tcr_detect_cfg* det, const uint8_t* reset, void* state, float* post, int32_t* top,
                                             float* score, int32_t* is_new, void* stream) {
    return phrase_stream_push("tcr_phrase_stream_push_ragged", true, n_streams, 0, step_offsets, total_steps, num_classes, values, n_phrases,
                              phrase_offsets, phrase_words, cfg, det, reset, state, post, top, score, is_new, stream);
}
