// Depthwise convolution of the generic 2-D layer-graph engine (net2d.cpp, node kind G2D_DWCONV): tf.nn.depthwise_conv2d with channel
// multiplier 1 -- slim.separable_conv2d(num_outputs=None, depth_multiplier=1) -- in the engine's layout, [B][C][h*w + 2*kHalo] with the
// plane at kHalo.  Weights [kh][kw][C][1]: tap (i, j) of channel c is wgt[(i*kw + j)*C + c].  Window, padding and output size are the
// dense conv's (net2d.cpp out_dim); any kernel / stride, dilation at stride 1, SAME or VALID, optional bias + ReLU.
//
// Included by net2d_kernels.hip (one translation unit); launchers are declared in net2d.h.
//
//   forward:  y[n][c][oh][ow]   = act(bias[c] + sum_{i,j} x[n][c][oh*sh + i*dh - pt][ow*sw + j*dw - pl] * W[i][j][c])
//   dgrad:    dx[n][c][ih][iw] += sum_{i,j} dy[n][c][(ih + pt - i*dh) / sh][(iw + pl - j*dw) / sw] * W[i][j][c]      (exact divisions only)
//   wgrad:    dW[i][j][c]       = sum_{n,oh,ow} x[n][c][oh*sh + i*dh - pt][ow*sw + j*dw - pl] * dy[n][c][oh][ow]
// with positions outside the plane contributing zero.  Every (utterance, channel) plane is independent and the layer is memory-bound:
// the forward / data gradient read their operand once into LDS and write their result once; no float atomics anywhere.
//
// Forward and data gradient are one kernel (DGRAD = false / true), a workgroup per (plane, tile of rows):
//   * the tile's rows of the launch's plane need a run of WHOLE rows of the gathered plane -- one contiguous range of floats -- which is
//     staged in LDS with 4-byte loads (no alignment is asked of any pointer); the row tile is sized so that the run fits, so the plane's
//     height is not limited by LDS;
//   * the channel is uniform per workgroup, so each tap is one scalar load per pass, held in an SGPR for the pass's outputs;
//   * every output is ONE fmaf chain from 0 over the taps in (i, then j) order, padding taps multiplying 0: its bits do not depend on
//     the tiling, the workgroup size or the order workgroups run in;
//   * bias and ReLU are fused into the forward's store; the data gradient accumulates (`+=`) into dx like launch_conv2d_dgrad,
//     each element owned by one thread.
// Two instances by workgroup size: 64 threads / 1024 staged floats when the whole plane is one tile of at most 256 outputs (the
// planes of small-footprint keyword spotters behind their first conv), 256 threads / 4096 floats otherwise.  The choice is made from the
// shapes alone.
#pragma once

namespace tcr {

constexpr int kDwRowTile = 32;          // rows of the launch's plane per tile (256-thread instance), fewer if the staged run would not fit
constexpr int kDwPerThread = 4;         // outputs a thread carries through one pass over the taps
constexpr int kDwLdsFloats = 4096;      // staged floats of the 256-thread instance (16 KB: LDS leaves room for 8 workgroups per CU)
constexpr int kDwSmallThreads = 64, kDwSmallLdsFloats = 1024, kDwSmallOutputs = kDwSmallThreads * kDwPerThread;

// rows of the gathered plane (height SH) that `rows` consecutive rows of the launch's plane can reach: an upper bound
static int dw2d_src_rows(bool dgrad, int rows, int k_eff, int stride, int SH) {
    const int need = dgrad ? rows + k_eff - 1 : (rows - 1) * stride + k_eff;
    return need < SH ? need : SH;
}

int dw2d_max_taps() { return 1024; }

// what one tile must be able to stage: a single row of the launch's plane, forward (the wider of the two gathered planes)
bool dw2d_fits(int k_eff_h, int h, int w) { return (int64_t)dw2d_src_rows(false, 1, k_eff_h, 1, h) * w <= kDwLdsFloats; }
int dw2d_lds_floats() { return kDwLdsFloats; }

// the launch geometry: threads per workgroup and rows per tile
static void dw2d_plan(const DwConv2dArgs& a, bool dgrad, int* threads, int* tile_rows) {
    const int PH = dgrad ? a.h : a.oh, PW = dgrad ? a.w : a.ow, SH = dgrad ? a.oh : a.h, SW = dgrad ? a.ow : a.w;
    const int k_eff = (a.kh - 1) * a.dh + 1;
    if ((int64_t)PH * PW <= kDwSmallOutputs && (int64_t)dw2d_src_rows(dgrad, PH, k_eff, a.sh, SH) * SW <= kDwSmallLdsFloats) {
        *threads = kDwSmallThreads; *tile_rows = PH;
        return;
    }
    int t = kDwRowTile;
    while (t > 1 && (int64_t)dw2d_src_rows(dgrad, t, k_eff, a.sh, SH) * SW > kDwLdsFloats) --t;
    *threads = 256; *tile_rows = t;
}

template <int NT, int LDS, bool DGRAD>
__global__ __launch_bounds__(NT) void dw2d_kernel(const DwConv2dArgs a, const int tile_rows) {
    __shared__ float s_src[LDS];
    const int plane_id = blockIdx.x;                                    // n * C + c
    const int ch = plane_id % a.c;
    const int PH = DGRAD ? a.h : a.oh, PW = DGRAD ? a.w : a.ow;         // plane the launch's positions enumerate
    const int SH = DGRAD ? a.oh : a.h, SW = DGRAD ? a.ow : a.w;         // plane the operand is gathered from
    const int spp = DGRAD ? a.ppo : a.ppi, dpp = DGRAD ? a.ppi : a.ppo;
    const int r0 = blockIdx.y * tile_rows, r1 = min(r0 + tile_rows, PH);
    // gathered rows the tile reaches, clipped to the plane
    int s_lo, s_hi;
    if (!DGRAD) {
        s_lo = r0 * a.sh - a.pt;
        s_hi = (r1 - 1) * a.sh - a.pt + (a.kh - 1) * a.dh;
    } else {
        const int t_lo = r0 + a.pt - (a.kh - 1) * a.dh;
        s_lo = t_lo > 0 ? (t_lo + a.sh - 1) / a.sh : 0;
        s_hi = (r1 - 1 + a.pt) / a.sh;
    }
    s_lo = max(s_lo, 0);
    s_hi = min(s_hi, SH - 1);
    const int nstage = s_hi >= s_lo ? (s_hi - s_lo + 1) * SW : 0;       // <= LDS: dw2d_plan sized tile_rows by dw2d_src_rows
    const float* src = a.x + (size_t)plane_id * spp + kHalo + (size_t)s_lo * SW;
    for (int e = threadIdx.x; e < nstage; e += NT) s_src[e] = src[e];
    __syncthreads();

    const float* wt = a.wgt + ch;                                       // tap stride: C
    const bool unit = a.sh == 1 && a.sw == 1;
    float* dst = a.y + (size_t)plane_id * dpp + kHalo;
    const float bias = (!DGRAD && a.bias) ? a.bias[ch] : 0.f;
    const int nout = (r1 - r0) * PW;
    for (int base = 0; base < nout; base += NT * kDwPerThread) {
        int py[kDwPerThread], px[kDwPerThread];
        float acc[kDwPerThread];
#pragma unroll
        for (int r = 0; r < kDwPerThread; ++r) {
            const int o = min(base + r * NT + (int)threadIdx.x, nout - 1);
            const int y = o / PW;
            py[r] = r0 + y;
            px[r] = o - y * PW;
            acc[r] = 0.f;
        }
        for (int i = 0; i < a.kh; ++i)
            for (int j = 0; j < a.kw; ++j) {
                const float wv = wt[(size_t)(i * a.kw + j) * a.c];
#pragma unroll
                for (int r = 0; r < kDwPerThread; ++r) {
                    int sy, sx;
                    bool ok;
                    if (!DGRAD) {
                        sy = py[r] * a.sh + i * a.dh - a.pt;
                        sx = px[r] * a.sw + j * a.dw - a.pl;
                        ok = sy >= 0 && sy < SH && sx >= 0 && sx < SW;
                    } else {
                        const int ty = py[r] + a.pt - i * a.dh, tx = px[r] + a.pl - j * a.dw;
                        sy = unit ? ty : ty / a.sh;                     // (stride 1, the common layer: no division)
                        sx = unit ? tx : tx / a.sw;
                        ok = ty >= 0 && tx >= 0 && sy * a.sh == ty && sx * a.sw == tx && sy < SH && sx < SW;
                    }
                    const float xv = s_src[ok ? (sy - s_lo) * SW + sx : 0];
                    acc[r] = fmaf(ok ? xv : 0.f, wv, acc[r]);
                }
            }
#pragma unroll
        for (int r = 0; r < kDwPerThread; ++r) {
            if (base + r * NT + (int)threadIdx.x >= nout) continue;
            float* o = dst + py[r] * PW + px[r];
            if (DGRAD) {
                o[0] += acc[r];                                         // gradient buffers accumulate (zeroed at the start of backward)
            } else {
                float v = acc[r] + bias;
                if (a.relu) v = fmaxf(v, 0.f);
                o[0] = v;
            }
        }
    }
}

template <bool DGRAD>
static int launch_dw2d_t(const DwConv2dArgs& a, const char* what, hipStream_t s) {
    const int64_t planes = (int64_t)a.batch * a.c;
    int threads, tile_rows;
    dw2d_plan(a, DGRAD, &threads, &tile_rows);
    const int tiles = ceil_div(DGRAD ? a.h : a.oh, tile_rows);
    // (the runtime takes at most 2^32 - 1 threads along a grid dimension: 2^24 planes of 256 threads, 2^26 of 64)
    if (planes * threads > (int64_t)0xffffffff || tiles > 65535) {
        set_error("%s: %lld planes of %d threads x %d row tiles exceed the launch geometry (batch x channels x threads < 2^32, tiles <= 65535)", what,
                  (long long)planes, threads, tiles);
        return TCR_ERR_ARG;
    }
    const dim3 grid((unsigned)planes, (unsigned)tiles);
    if (threads == kDwSmallThreads) hipLaunchKernelGGL((dw2d_kernel<kDwSmallThreads, kDwSmallLdsFloats, DGRAD>), grid, dim3(kDwSmallThreads), 0, s, a, tile_rows);
    else hipLaunchKernelGGL((dw2d_kernel<256, kDwLdsFloats, DGRAD>), grid, dim3(256), 0, s, a, tile_rows);
    return check_launch(what);
}

int launch_dw2d_fwd(const DwConv2dArgs& a, hipStream_t s) { return launch_dw2d_t<false>(a, "dw2d_fwd_kernel", s); }
int launch_dw2d_dgrad(const DwConv2dArgs& a, hipStream_t s) { return launch_dw2d_t<true>(a, "dw2d_dgrad_kernel", s); }

// ---- filter gradient --------------------------------------------------------------------------------------------------------
// partial[chunk][tap][c] = sum over the chunk's utterances and all output positions of x[c][in(pos, tap)] * dy[c][pos].
// A workgroup per (channel, utterance chunk); each of its four waves takes every fourth tap, its lanes stride the chunk's
// (utterance, position) pairs in a fixed order and the 64 lane sums are folded by a butterfly: the same bits on every run.  The chunks
// (conv2d_wgrad_chunks, as for the dense conv) are then summed in a fixed order by launch_wgrad_reduce ([tap][1][C] slabs).
__global__ __launch_bounds__(256) void dw2d_wgrad_kernel(const DwConv2dArgs a, float* __restrict__ partial, const int utt_per_block) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ch = blockIdx.x, chunk = blockIdx.y;
    const int n0 = chunk * utt_per_block, n1 = min(n0 + utt_per_block, a.batch);
    const int oplane = a.oh * a.ow, taps = a.kh * a.kw;
    const int total = (n1 - n0) * oplane;                               // (< 2^31: launch_dw2d_wgrad)
    for (int tap = wave; tap < taps; tap += 4) {
        const int ti = tap / a.kw, tj = tap - ti * a.kw;
        float acc = 0.f;
        for (int e = lane; e < total; e += 64) {
            const int n = e / oplane, p = e - n * oplane;
            const int oy = p / a.ow, ox = p - oy * a.ow;
            const int sy = oy * a.sh + ti * a.dh - a.pt, sx = ox * a.sw + tj * a.dw - a.pl;
            const bool ok = sy >= 0 && sy < a.h && sx >= 0 && sx < a.w;
            const size_t row = (size_t)(n0 + n) * a.c + ch;
            const float xv = a.x[row * a.ppi + kHalo + (ok ? sy * a.w + sx : 0)];
            const float dv = a.dy[row * a.ppo + kHalo + p];
            acc = fmaf(ok ? xv : 0.f, dv, acc);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
        if (lane == 0) partial[((size_t)chunk * taps + tap) * a.c + ch] = acc;
    }
}

size_t dw2d_wgrad_partial_floats(int kh, int kw, int c, int batch) { return (size_t)conv2d_wgrad_chunks(batch) * kh * kw * c; }

int launch_dw2d_wgrad(const DwConv2dArgs& a, float* dw, float* scratch, hipStream_t s) {
    const int upb = ceil_div(a.batch, conv2d_wgrad_chunks(a.batch));
    const int nchunk = ceil_div(a.batch, upb);
    const int taps = a.kh * a.kw;
    if ((int64_t)upb * a.oh * a.ow >= ((int64_t)1 << 31) - 64 || nchunk > 65535 || (int64_t)a.c * 256 > (int64_t)0xffffffff) {
        set_error("dw2d wgrad: %d utterances x %d positions per chunk exceed the launch geometry", upb, a.oh * a.ow);
        return TCR_ERR_ARG;
    }
    hipLaunchKernelGGL(dw2d_wgrad_kernel, dim3((unsigned)a.c, (unsigned)nchunk), dim3(256), 0, s, a, scratch, upb);
    TCR_TRY(check_launch("dw2d_wgrad_kernel"));
    return launch_wgrad_reduce(scratch, dw, nchunk, taps, 1, a.c, 1, a.c, a.c, 0, s);
}

}  // namespace tcr
