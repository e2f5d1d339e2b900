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

// Dynamic LDS: the staged columns [U][TILE + w - 1].  No static LDS; see profiles/phrase_kernel_regs.txt for registers and scratch.
template <bool RAGGED>
__global__ __launch_bounds__(256) void phrase_kernel(const PhraseArgs a) {
    float* s_p = reinterpret_cast<float*>(dyn_lds());
    const int tid = threadIdx.x, C = a.C, P = a.P;
    int64_t row0, i0, len_sig;
    if constexpr (RAGGED) {
        const int64_t b = blockIdx.x;
        int lo = 0, hi = a.N - 1;                       // the last n with step_off[n] / TILE + n <= b
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.step_off[mid] / kPhraseTile + mid <= b) lo = mid;
            else hi = mid - 1;
        }
        row0 = a.step_off[lo];
        len_sig = a.step_off[lo + 1] - row0;
        i0 = (b - (row0 / kPhraseTile + lo)) * kPhraseTile;
    } else {
        const int64_t n = blockIdx.x / (uint64_t)a.tiles;
        row0 = n * a.steps;
        len_sig = a.steps;
        i0 = (blockIdx.x - n * a.tiles) * kPhraseTile;
    }
    if (i0 >= len_sig) return;                          // (ragged: a signal without steps, or a spare block)
    const int len = (int)(len_sig - i0 < kPhraseTile ? len_sig - i0 : kPhraseTile);
    const int h = (int)(i0 < a.w - 1 ? i0 : a.w - 1);   // rows in front of the tile (never before the signal's first)
    const float* src = a.values + (row0 + i0 - h) * C;
    const int n_rows = h + len;                         // <= stride
    for (int u = 0; u < a.U; ++u) {
        const int cls = a.col_class[u];
        float* dst = s_p + u * a.stride;
        for (int s = tid; s < n_rows; s += 256) dst[s] = src[(int64_t)s * C + cls];
    }
    __syncthreads();
    if (tid >= len) return;                             // (after the kernel's only barrier)
    const int64_t i = i0 + tid;
    const int count = i + 1 < a.w ? (int)(i + 1) : a.w;
    const float* s_at = s_p + (h + tid - count + 1);    // >= s_p: count = i + 1 while h = i0, else h = w - 1 = count - 1
    float* o = a.out + (row0 + i) * (P + 1);
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

namespace {

int phrase_scores(const char* what, bool ragged, int n_signals, int64_t steps, const int64_t* step_offsets, int64_t total_steps, int num_classes,
                  const float* values, int n_phrases, const int32_t* phrase_offsets, const int32_t* phrase_words, const tcr_phrase_cfg* cfg,
                  float* out, void* stream) {
    TCR_REQUIRE((!ragged || step_offsets) && values && phrase_offsets && phrase_words && cfg && out, "%s: null argument", what);
    TCR_REQUIRE(n_signals > 0, "%s: the number of signals must be positive (got %d)", what, n_signals);
    TCR_REQUIRE(ragged ? total_steps > 0 : steps > 0, "%s: the number of steps must be positive (got %lld)", what,
                (long long)(ragged ? total_steps : steps));
    TCR_REQUIRE(num_classes > 0, "%s: num_classes must be positive (got %d)", what, num_classes);
    TCR_REQUIRE(n_phrases >= 1 && n_phrases <= kPhraseMax, "%s: n_phrases %d outside 1..%d", what, n_phrases, kPhraseMax);
    TCR_REQUIRE(phrase_offsets[0] == 0, "%s: phrase_offsets must start at 0 (got %d)", what, phrase_offsets[0]);
    PhraseArgs a{};
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
    const int64_t rows = ragged ? total_steps : steps * n_signals;
    const int widest = num_classes > n_phrases + 1 ? num_classes : n_phrases + 1;
    TCR_REQUIRE((ragged || steps < ((int64_t)1 << 31)) && rows < ((int64_t)1 << 31) && rows * widest < ((int64_t)1 << 31),
                "%s: %lld steps in all x %d columns is too large", what, (long long)rows, widest);
    a.values = values; a.out = out; a.step_off = ragged ? step_offsets : nullptr;
    a.steps = steps; a.tiles = ragged ? 0 : ceil_div64(steps, kPhraseTile);
    a.N = n_signals; a.C = num_classes; a.P = n_phrases; a.U = U; a.w = cfg->window_steps; a.stride = kPhraseTile + cfg->window_steps - 1;
    a.ordered = cfg->ordered; a.combine = cfg->combine;
    const int64_t blocks = ragged ? total_steps / kPhraseTile + n_signals : a.tiles * n_signals;
    const size_t lds = (size_t)a.stride * U * sizeof(float);
    const auto kernel = ragged ? phrase_kernel<true> : phrase_kernel<false>;
    if (lds > 32 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
                               hipSuccess) {
        set_error("%s: hipFuncSetAttribute failed", what);
        return TCR_ERR_HIP;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, static_cast<hipStream_t>(stream), a);
    return check_launch("phrase_kernel");
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
