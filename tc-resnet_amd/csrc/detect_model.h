// The network of the detection entries (tcr_stream_*, tcr_scan, tcr_stream_scan and their _m twins): one dispatch point per
// model family for the input shape, the workspace at a batch and the forward, so that stream.hip / scan.hip never
// name a family's entry themselves.
//
// The windows a detection call hands the network are always the front-end's planar [n_coef][T + 2 TCR_HALO] rows, except for the
// 2-D graph, which reads one [T x n_coef] plane per window ([B][1][T n_coef + 2 TCR_HALO], tcr_g2d_input_from_features's layout:
// plane offset t n_coef + c <- window column t, coefficient c).  The scan / push parity rests on every family's result for a window
// not depending on its batch: TC-ResNet (DESIGN, net_small_tc8_kernel), DS-CNN up to kDscnnMaxBatch (below), the 2-D graphs
// (tests/test_detect_families.py checks both at batches 1 .. 4096).
//
// Compiled as part of frontend_pk3.hip's translation unit (included by stream.hip).
#pragma once
#include <climits>

#include "tcr_common.h"

namespace tcr {

namespace {

// launch_dscnn_conv1_dw (dscnn.hip) runs its fused conv_1 + depthwise kernel up to this batch and another path above it: the
// detection entries keep every DS-CNN launch at or below it, so that every window takes the same path.
constexpr int kDscnnMaxBatch = 65535 * 16;

struct ModelIO {
    int n_coef = 0, t = 0, classes = 0;     // the input the front-end must yield (n_coef x T) and the classes
    bool planes = false;                    // the network reads [T x n_coef] planes (2-D graph), not planar windows
    int max_batch = INT_MAX;                // the largest batch one network call may run
};

// Family, finalization and shape of a non-null reference with a non-null handle.
int model_io(const tcr_model_ref& m, const char* what, ModelIO& io) {
    io = ModelIO();
    switch (m.family) {
        case TCR_FAMILY_TCRESNET:
            net_io_shape(static_cast<const tcr_net*>(m.handle), &io.n_coef, &io.t, &io.classes);
            return TCR_OK;
        case TCR_FAMILY_DSCNN:
            dscnn_io_shape(static_cast<const tcr_dscnn*>(m.handle), &io.n_coef, &io.t, &io.classes);
            io.max_batch = kDscnnMaxBatch;
            return TCR_OK;
        case TCR_FAMILY_G2D: {
            int c = 0;
            const bool fin = g2d_io_shape(static_cast<const tcr_g2d*>(m.handle), &c, &io.t, &io.n_coef, &io.classes);
            TCR_REQUIRE(fin, "%s: the 2-D graph is not finalized (tcr_g2d_finalize)", what);
            TCR_REQUIRE(c == 1, "%s: the 2-D graph's input has %d channels; the detector feeds it one [T x n_coef] feature plane", what, c);
            io.planes = true;
            return TCR_OK;
        }
        default:
            set_error("%s: unknown model family %d (TCR_FAMILY_TCRESNET, TCR_FAMILY_DSCNN or TCR_FAMILY_G2D)", what, m.family);
            return TCR_ERR_ARG;
    }
}

// floats of one window as the network reads it
int64_t model_window_floats(const ModelIO& io) {
    return io.planes ? (int64_t)io.t * io.n_coef + 2 * kHalo : (int64_t)io.n_coef * tcr_padded_len(io.t);
}

size_t model_workspace_bytes(const tcr_model_ref& m, int batch) {
    switch (m.family) {
        case TCR_FAMILY_DSCNN: return tcr_dscnn_workspace_bytes(static_cast<const tcr_dscnn*>(m.handle), batch);
        case TCR_FAMILY_G2D: return tcr_g2d_workspace_bytes(static_cast<const tcr_g2d*>(m.handle), batch, 0);
        default: return tcr_net_workspace_bytes(static_cast<const tcr_net*>(m.handle), batch, 0);
    }
}

// the eval forward of `batch` windows x (model_window_floats each)
int model_forward(const tcr_model_ref& m, const float* x, int batch, float* ws, size_t ws_bytes, float* logits, float* probs, void* stream) {
    switch (m.family) {
        case TCR_FAMILY_DSCNN:
            return tcr_dscnn_forward_infer(static_cast<const tcr_dscnn*>(m.handle), m.params, m.aux, x, batch, ws, ws_bytes, logits, probs,
                                           stream);
        case TCR_FAMILY_G2D:
            return tcr_g2d_forward_infer(static_cast<const tcr_g2d*>(m.handle), m.params, m.aux, x, batch, ws, ws_bytes, logits, probs,
                                         stream);
        default:
            return tcr_net_forward_frozen(static_cast<const tcr_net*>(m.handle), m.params, m.aux, x, batch, ws, ws_bytes, logits, probs,
                                          nullptr, stream);
    }
}

// the reference the entries without _m stand for
tcr_model_ref tcresnet_ref(const tcr_net* net, const float* params, const float* frozen_ss) {
    tcr_model_ref m;
    m.family = TCR_FAMILY_TCRESNET;
    m.handle = net;
    m.params = params;
    m.aux = frozen_ss;
    return m;
}

}  // namespace

}  // namespace tcr
