// Sample-rate conversion (tcr_resample): a rational-ratio polyphase FIR, int16 PCM or float32 in, float32 out -- the stage in front of
// the detectors, which take float32 at the model's rate.  Stateless: every output is a pure function of its global index.
//
// up = L, down = M (coprime), taps = P, table float32 [L][P].  Output j (global index, int64):
//     n_j = floor(j M / L),  phi_j = (j M) mod L,  lead = P / 2 - 1 (0 when P == 1)
//     y[j] = fmaf chain over p = 0 .. P - 1, in this order, from 0:  table[phi_j][p] * x[n_j - lead + p]
// x[i] is the decoded input at global index i (int16: (float)v * (1 / 32768), exact), 0 outside the span the caller passed.  The
// order of the chain is fixed, so a sample's value does not depend on the tile, the chunk or the launch that computed it.
//
// With j = q L + r (0 <= r < L):  n_j = q M + floor(r M / L)  and  phi_j = (r M) mod L  -- no 64-bit division per output, and the
// outputs of one residue r share one table row.  resample_kernel: a workgroup owns, for one stream, B consecutive q and G consecutive
// residues r (G = L when L is small: consecutive outputs).  It stages
//   the G table rows (pitch P | 1: the rows of a 32-lane group then fall on different LDS banks),
//   the input span the tile reads, (B - 1) M + floor((r0 + G - 1) M / L) - floor(r0 M / L) + P samples, decoded to float32,
//   zeros outside the rows, the in_step stride (interleaved channels) applied here,
// and each thread walks the P taps of four outputs of one row from LDS, four independent fmaf chains fed by one coefficient read (b
// fastest over the lanes: at L = 1 lane l starts M words after lane l - 1).  A table of many rows (44.1 kHz -> 16 kHz: 160 x 178)
// never sits in LDS whole: a workgroup holds the G <= 32 rows of its residues, and L / G workgroups share one input span through L2.
// At most 80.3 KB of LDS (24 KB of rows + 56 KB of samples + the 64 per-row ints): G = min(L, 32, 6144 / (P | 1)) rows, and the host
// refuses (TCR_ERR_ARG, before any HIP call) what cannot be staged -- P > 6143 (no row fits), or one q of a row group beyond the span,
// P + ceil(G M / L) + 1 > 14336 -- so no accepted configuration asks for more.
//
// Compiled as part of frontend_pk3.hip's translation unit (included at its end, after sweep.hip).
#pragma once
#include <algorithm>

namespace tcr {

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsMaxRows = 32;                          // G: table rows per workgroup at most
constexpr int kRsTableFloats = 6144;                    // G (P | 1) <= this (24 KB)
constexpr int kRsSpanFloats = 14336;                    // staged input samples per workgroup at most (56 KB)
constexpr int kRsTileOutputs = 1024;                    // G B aimed at (four outputs per thread)

inline int64_t floor_div64(int64_t a, int64_t b) {      // b > 0
    int64_t q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

}  // namespace

struct ResampleArgs {
    const float* table;         // [L][P]
    const void* in;
    float* out;
    int64_t in_pitch, in_first, n_in, out_first, n_out, out_pitch;
    int64_t q_lo;               // floor(out_first / L): the first tile's first q
    int L, M, P, lead, in_format, in_step;
    int G, B, pitch;            // rows and q per workgroup, LDS pitch of a table row
    int span_cap;               // LDS floats of the span region
    int s0;                     // the launch's first stream
};

// Dynamic LDS: table rows [G][pitch] | samples [span] | per-row first-sample offsets and table rows int [2][kRsMaxRows].
__global__ __launch_bounds__(kRsThreads) void resample_kernel(const ResampleArgs a) {
    float* s_tab = reinterpret_cast<float*>(dyn_lds());
    float* s_x = s_tab + a.G * a.pitch;
    int* s_off = reinterpret_cast<int*>(s_x + a.span_cap);
    const int tid = threadIdx.x;
    const int s = a.s0 + (int)blockIdx.z;
    const int r0 = (int)blockIdx.y * a.G;
    const int G = a.L - r0 < a.G ? a.L - r0 : a.G;      // (the last row group may be short)
    const int64_t q0 = a.q_lo + (int64_t)blockIdx.x * a.B;
    const int64_t f0 = (int64_t)r0 * a.M / a.L;         // floor(r0 M / L)
    int* s_phi = s_off + kRsMaxRows;
    if (tid < G) {
        s_off[tid] = (int)((int64_t)(r0 + tid) * a.M / a.L - f0);
        s_phi[tid] = (int)((int64_t)(r0 + tid) * a.M % a.L);
    }
    __syncthreads();
    for (int e = tid; e < G * a.P; e += kRsThreads) {
        const int k = e / a.P, p = e - k * a.P;
        s_tab[k * a.pitch + p] = a.table[(int64_t)s_phi[k] * a.P + p];
    }
    // the span: global input indices x0 .. x0 + span - 1
    const int64_t x0 = q0 * a.M + f0 - a.lead;
    const int span = (int)((int64_t)(a.B - 1) * a.M + ((int64_t)(r0 + G - 1) * a.M / a.L - f0) + a.P);
    const int64_t row = (int64_t)s * a.in_pitch;
    for (int e = tid; e < span; e += kRsThreads) {
        const int64_t i = x0 + e - a.in_first;
        float v = 0.f;
        if (i >= 0 && i < a.n_in) {
            const int64_t at = row + i * a.in_step;
            v = a.in_format ? (float)static_cast<const int16_t*>(a.in)[at] * (1.0f / 32768.0f) : static_cast<const float*>(a.in)[at];
        }
        s_x[e] = v;
    }
    __syncthreads();
    float* out = a.out + (int64_t)s * a.out_pitch;
    const int P = a.P, Bq = (a.B + 3) >> 2;
    // a unit: row k and outputs b, b + Bq, b + 2 Bq, b + 3 Bq of it -- one coefficient read feeds four independent chains
    for (int u = tid; u < G * Bq; u += kRsThreads) {
        const int k = u / Bq, bb = u - k * Bq;
        const float* c = s_tab + k * a.pitch;
        const float* x[4];
        int64_t j[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int b = bb + i * Bq;
            j[i] = (q0 + b) * a.L + r0 + k - a.out_first;
            if (b >= a.B || j[i] < 0 || j[i] >= a.n_out) j[i] = -1;
            x[i] = s_x + (j[i] < 0 ? 0 : b * a.M + s_off[k]);              // (not an output: reads the span's first P samples, stores nothing)
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int p = 0; p < P; ++p) {
            const float cp = c[p];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(cp, x[i][p], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (j[i] >= 0) out[j[i]] = acc[i];
    }
}

}  // namespace tcr

using namespace tcr;

namespace {

int resample_cfg_check(const tcr_resample_cfg* cfg, const char* who) {
    TCR_REQUIRE(cfg, "%s: null cfg", who);
    TCR_REQUIRE(cfg->up >= 1 && cfg->down >= 1 && cfg->taps >= 1, "%s: up, down and taps must be >= 1 (got %d, %d, %d)", who, cfg->up,
                cfg->down, cfg->taps);
    TCR_REQUIRE(cfg->taps == 1 || cfg->taps % 2 == 0, "%s: taps must be even or 1 (got %d)", who, cfg->taps);
    TCR_REQUIRE(cfg->in_format == 0 || cfg->in_format == 1, "%s: unknown in_format %d (0 float32, 1 int16)", who, cfg->in_format);
    TCR_REQUIRE(cfg->in_step >= 1, "%s: in_step must be >= 1 (got %d)", who, cfg->in_step);
    return TCR_OK;
}

// |j| * down stays inside int64 with room for the tile arithmetic
bool resample_range_ok(const tcr_resample_cfg* cfg, int64_t out_first, int64_t n_out) {
    const int64_t lim = ((int64_t)1 << 61) / cfg->down;
    return out_first > -lim && out_first < lim && n_out < lim && out_first + n_out < lim;
}

}  // namespace

extern "C" int tcr_resample_span(const tcr_resample_cfg* cfg, int64_t out_first, int64_t n_out, int64_t* first, int64_t* n) {
    TCR_TRY(resample_cfg_check(cfg, "tcr_resample_span"));
    TCR_REQUIRE(first && n, "tcr_resample_span: null argument");
    TCR_REQUIRE(n_out >= 0, "tcr_resample_span: n_out must be >= 0 (got %lld)", (long long)n_out);
    TCR_REQUIRE(resample_range_ok(cfg, out_first, n_out), "tcr_resample_span: outputs %lld + %lld are out of range", (long long)out_first,
                (long long)n_out);
    const int lead = cfg->taps > 1 ? cfg->taps / 2 - 1 : 0;
    *first = floor_div64(out_first * cfg->down, cfg->up) - lead;
    *n = n_out == 0 ? 0 : floor_div64((out_first + n_out - 1) * cfg->down, cfg->up) - lead + cfg->taps - *first;
    return TCR_OK;
}

extern "C" int tcr_resample(const tcr_resample_cfg* cfg, const float* table, int n_streams, const void* in, int64_t in_pitch,
                            int64_t in_first, int64_t n_in, int64_t out_first, int64_t n_out, float* out, int64_t out_pitch,
                            void* stream) {
    TCR_TRY(resample_cfg_check(cfg, "tcr_resample"));
    TCR_REQUIRE(table && in && out, "tcr_resample: null argument");
    TCR_REQUIRE(n_streams >= 0 && n_in >= 0 && n_out >= 0, "tcr_resample: negative count (S %d, n_in %lld, n_out %lld)", n_streams,
                (long long)n_in, (long long)n_out);
    TCR_REQUIRE(n_in < ((int64_t)1 << 61) / cfg->in_step, "tcr_resample: n_in %lld is out of range", (long long)n_in);
    TCR_REQUIRE(in_pitch >= (n_in > 0 ? (n_in - 1) * cfg->in_step + 1 : 0), "tcr_resample: in_pitch %lld is smaller than a row of %lld samples",
                (long long)in_pitch, (long long)n_in);
    TCR_REQUIRE(out_pitch >= n_out, "tcr_resample: out_pitch %lld is smaller than a row of %lld samples", (long long)out_pitch, (long long)n_out);
    TCR_REQUIRE(resample_range_ok(cfg, out_first, n_out) && in_first > -((int64_t)1 << 61) && in_first < ((int64_t)1 << 61),
                "tcr_resample: positions out of range (out_first %lld, n_out %lld, in_first %lld)", (long long)out_first, (long long)n_out,
                (long long)in_first);
    ResampleArgs a;
    a.L = cfg->up; a.M = cfg->down; a.P = cfg->taps; a.lead = cfg->taps > 1 ? cfg->taps / 2 - 1 : 0;
    a.in_format = cfg->in_format; a.in_step = cfg->in_step;
    // tile: G rows (their LDS image within kRsTableFloats), then as many q as the span allows, G B about kRsTileOutputs
    a.pitch = a.P | 1;
    a.G = std::min(std::min(a.L, kRsMaxRows), kRsTableFloats / a.pitch);
    TCR_REQUIRE(a.G >= 1, "tcr_resample: %d taps per phase are more than the kernel stages (%d)", a.P, kRsTableFloats - 1);
    const int64_t rows_span = ((int64_t)a.G * a.M + a.L - 1) / a.L + 1;          // >= floor((r0 + G - 1) M / L) - floor(r0 M / L) + 1
    // one q (B = 1) must fit: rows_span + P <= kRsSpanFloats.  (Asked of the sum, not of b_fit: a deficit below M truncates to b_fit = 1.)
    TCR_REQUIRE(a.P + rows_span <= kRsSpanFloats, "tcr_resample: %d taps at %d : %d need more than the %d samples a workgroup stages", a.P,
                a.L, a.M, kRsSpanFloats);
    const int64_t b_fit = (kRsSpanFloats - a.P - rows_span) / a.M + 1;            // (B - 1) M + rows_span + P <= kRsSpanFloats
    a.B = (int)std::min<int64_t>(b_fit, std::max(1, kRsTileOutputs / a.G));
    if (a.B > 4) a.B &= ~3;                                                        // (whole four-chain units)
    if (n_out == 0 || n_streams == 0) return TCR_OK;
    const int64_t groups = (a.L + a.G - 1) / a.G;
    TCR_REQUIRE(groups <= 65535, "tcr_resample: up = %d has more phase groups than one launch covers", a.L);
    a.q_lo = floor_div64(out_first, a.L);
    const int64_t tiles = (floor_div64(out_first + n_out - 1, a.L) - a.q_lo) / a.B + 1;
    TCR_REQUIRE(tiles < ((int64_t)1 << 31), "tcr_resample: %lld outputs are more than one call covers", (long long)n_out);
    a.table = table; a.in = in; a.out = out;
    a.in_pitch = in_pitch; a.in_first = in_first; a.n_in = n_in; a.out_first = out_first; a.n_out = n_out; a.out_pitch = out_pitch;
    a.span_cap = (int)((a.B - 1) * (int64_t)a.M + rows_span + a.P + 3) / 4 * 4;
    const size_t lds = ((size_t)a.G * a.pitch + a.span_cap + 2 * kRsMaxRows) * sizeof(float);
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        set_error("tcr_resample: hipFuncSetAttribute failed");
        return TCR_ERR_HIP;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int s0 = 0; s0 < n_streams; s0 += 65535) {
        a.s0 = s0;
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, (unsigned)groups, (unsigned)std::min(65535, n_streams - s0)),
                           dim3(kRsThreads), lds, st, a);
        TCR_TRY(check_launch("resample_kernel"));
    }
    return TCR_OK;
}
