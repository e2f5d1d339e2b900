"""Times the depthwise node of the 2-D graph engine (csrc/net2d_dw.hip) on the GPU and writes profiles/g2d_depthwise_bench.json.

Per shape at batch 4096 -- DS-CNN-L's two block shapes (276 channels: the first block's 25 x 10 plane at stride 2 x 2, the others' 13 x 5
at stride 1) and a 9 x 1 temporal kernel over 49 x 1 with 64 channels -- the forward, data-gradient and filter-gradient launchers
(launch_dw2d_fwd / _dgrad / _wgrad, the last with its chunk reduction) between device events, warmed, over enough launches for a window
of at least 0.2 s; each as achieved bytes/s over (x read + y written) computed from the shapes, next to a device-to-device copy of the
same bytes and to torch.nn.functional.conv2d(groups=C) and its two gradient functions on the device.  Then DS-CNN-L as a graph twin
(audio_nets/ds_cnn.py) against engine.DSCNN("L"), alternating in the same run: eval forward and one training step (forward, backward,
Adam) at batch 4096.

    python scripts/g2d_depthwise_bench.py [--batch 4096] [--out profiles/g2d_depthwise_bench.json]

The launchers are C++ functions of the library (not C ABI): they are called by their mangled names with a mirror of DwConv2dArgs."""
import argparse
import ctypes as C
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tcresnet_amd as T  # noqa: E402

HALO = T._lib.HALO
FWD = "_ZN3tcr15launch_dw2d_fwdERKNS_12DwConv2dArgsEP12ihipStream_t"
DGRAD = "_ZN3tcr17launch_dw2d_dgradERKNS_12DwConv2dArgsEP12ihipStream_t"
WGRAD = "_ZN3tcr17launch_dw2d_wgradERKNS_12DwConv2dArgsEPfS3_P12ihipStream_t"
PARTIAL = "_ZN3tcr25dw2d_wgrad_partial_floatsEiiii"


class DwArgs(C.Structure):          # csrc/net2d.h DwConv2dArgs
    _fields_ = [("x", C.c_void_p), ("wgt", C.c_void_p), ("y", C.c_void_p), ("bias", C.c_void_p), ("dy", C.c_void_p)] + \
               [(n, C.c_int) for n in "batch c h w oh ow kh kw sh sw dh dw pt pl ppi ppo relu".split()]


def out_dim(length, k, stride):
    out = -(-length // stride)
    return out, max((out - 1) * stride + k - length, 0) // 2


def timed(fn, min_seconds=0.2):
    """Median of 5 windows of n launches between device events, n sized so that a window lasts min_seconds; seconds per launch."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    n = max(3, int(min_seconds * 1e3 / max(a.elapsed_time(b), 1e-3)))
    per = []
    for _ in range(5):
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1e-3 / n)
    per.sort()
    return {"seconds": per[2], "min": per[0], "max": per[4], "launches_per_window": n}


def bench_shape(dll, name, batch, c, h, w, k, stride):
    dev = torch.device("cuda")
    (oh, pt), (ow, pl) = out_dim(h, k[0], stride[0]), out_dim(w, k[1], stride[1])
    ppi, ppo = h * w + 2 * HALO, oh * ow + 2 * HALO
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn((batch, c, ppi), generator=g).to(dev)
    dy = torch.randn((batch, c, ppo), generator=g).to(dev)
    y, dx = torch.zeros_like(dy), torch.zeros_like(x)
    wgt = torch.randn((k[0] * k[1], c), generator=g).to(dev)
    bias = torch.randn((c,), generator=g).to(dev)
    dwt = torch.zeros_like(wgt)
    dll[PARTIAL].restype = C.c_size_t
    scratch = torch.zeros((dll[PARTIAL](k[0], k[1], c, batch),), device=dev)
    base = dict(batch=batch, c=c, h=h, w=w, oh=oh, ow=ow, kh=k[0], kw=k[1], sh=stride[0], sw=stride[1], dh=1, dw=1, pt=pt, pl=pl, ppi=ppi, ppo=ppo, relu=1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fa = DwArgs(x=x.data_ptr(), wgt=wgt.data_ptr(), y=y.data_ptr(), bias=bias.data_ptr(), dy=None, **base)
    da = DwArgs(x=dy.data_ptr(), wgt=wgt.data_ptr(), y=dx.data_ptr(), bias=None, dy=None, **base)
    wa = DwArgs(x=x.data_ptr(), wgt=wgt.data_ptr(), y=None, bias=None, dy=dy.data_ptr(), **base)

    def call(sym, *a):
        rc = dll[sym](*a)
        assert rc == 0, (sym, rc)
    nbytes = batch * c * (h * w + oh * ow) * 4           # x read + y written (the data gradient: dy read + dx written; it also reads dx)
    res = {"shape": dict(batch=batch, c=c, h=h, w=w, oh=oh, ow=ow, kernel=list(k), stride=list(stride)), "bytes_x_plus_y": nbytes}
    for what, fn in (("forward", lambda: call(FWD, C.byref(fa), stream)), ("data_gradient", lambda: call(DGRAD, C.byref(da), stream)),
                     ("filter_gradient", lambda: call(WGRAD, C.byref(wa), C.c_void_p(dwt.data_ptr()), C.c_void_p(scratch.data_ptr()), stream))):
        t = timed(fn)
        t["bytes_per_second"] = nbytes / t["seconds"]
        res[what] = t
    # correctness of what was timed, against torch on the device
    xt = x[:, :, HALO:HALO + h * w].reshape(batch, c, h, w)
    wt = wgt.t().reshape(c, 1, k[0], k[1]).contiguous()
    pads = (pl, max((ow - 1) * stride[1] + k[1] - w, 0) - pl, pt, max((oh - 1) * stride[0] + k[0] - h, 0) - pt)
    xp = F.pad(xt, pads).contiguous()
    ref = F.relu(F.conv2d(xp, wt, bias, stride=stride, groups=c))
    got = y[:, :, HALO:HALO + oh * ow].reshape(batch, c, oh, ow)
    res["forward_max_abs_diff_vs_torch"] = float((got - ref).abs().max())
    # DwArgs mirrors a C++ struct by hand: every launcher's result is checked against torch, so a field that moved shows here and
    # not as a wrong time.  Relative to the largest reference value; float32 sums of at most batch x plane terms.
    dyt = dy[:, :, HALO:HALO + oh * ow].reshape(batch, c, oh, ow).contiguous()
    dx.zero_()
    call(DGRAD, C.byref(da), stream)
    ref_dx = torch.nn.grad.conv2d_input(xp.shape, wt, dyt, stride=stride, groups=c)[:, :, pads[2]:pads[2] + h, pads[0]:pads[0] + w]
    got_dx = dx[:, :, HALO:HALO + h * w].reshape(batch, c, h, w)
    call(WGRAD, C.byref(wa), C.c_void_p(dwt.data_ptr()), C.c_void_p(scratch.data_ptr()), stream)
    ref_dw = torch.nn.grad.conv2d_weight(xp, wt.shape, dyt, stride=stride, groups=c).reshape(c, k[0], k[1])
    got_dw = dwt.t().reshape(c, k[0], k[1])
    rel = lambda a_, b_: float((a_ - b_).abs().max() / b_.abs().max())
    res["data_gradient_rel_diff_vs_torch"], res["filter_gradient_rel_diff_vs_torch"] = rel(got_dx, ref_dx), rel(got_dw, ref_dw)
    assert res["forward_max_abs_diff_vs_torch"] < 1e-4 * max(1.0, float(ref.abs().max())), res["forward_max_abs_diff_vs_torch"]
    assert res["data_gradient_rel_diff_vs_torch"] < 1e-4 and res["filter_gradient_rel_diff_vs_torch"] < 1e-3, res
    dx.zero_()
    # a device-to-device copy moving the same bytes (half read, half written)
    src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src))
    t["bytes_per_second"] = nbytes / t["seconds"]
    res["device_copy"] = t
    # torch.nn.functional.conv2d(groups=C) on the padded plane, and its gradient functions
    try:
        for what, fn in (("torch_forward", lambda: F.conv2d(xp, wt, None, stride=stride, groups=c)),
                         ("torch_data_gradient", lambda: torch.nn.grad.conv2d_input(xp.shape, wt, dyt, stride=stride, groups=c)),
                         ("torch_filter_gradient", lambda: torch.nn.grad.conv2d_weight(xp, wt.shape, dyt, stride=stride, groups=c))):
            t = timed(fn)
            t["bytes_per_second"] = nbytes / t["seconds"]
            res[what] = t
    except Exception as e:          # noqa: BLE001
        res["torch"] = f"not measured: {type(e).__name__}: {str(e)[:200]}"
    print(name, json.dumps({k_: (v["seconds"] if isinstance(v, dict) and "seconds" in v else None) for k_, v in res.items()}), flush=True)
    return res


def bench_twin(batch):
    """DS-CNN-L: the graph twin and the dedicated engine, alternating: eval forward, one training step (forward, backward, Adam)."""
    from tcresnet_amd.audio_nets import ds_cnn
    dev = torch.device("cuda")
    lib = T._lib.get()
    twin = ds_cnn.build_graph(276, 5, "10x4", "2x1", "3x3", "2x2", "1x1", 49, 10, 12, lib=lib, device=dev)
    eng = T.DSCNN("L", 49, 10, 12, lib=lib, device=dev)
    eng.init_xavier(0)
    twin.load_state_dict(eng.state_dict())
    g = torch.Generator().manual_seed(2)
    feat = T.features_to_planar(torch.randn((batch, 49, 10), generator=g).to(dev), lib=lib)
    labels = F.one_hot(torch.randint(0, 12, (batch,), generator=g), 12).float().to(dev)
    a, b = twin.forward_infer(feat)[0], eng.forward_infer(feat)[0]
    res = {"batch": batch, "eval_logits_max_abs_diff": float((a - b).abs().max())}

    def step(net):
        net.forward_train(feat, labels)
        net.backward()
        net.adam_step(1e-4, 1)
    rounds = {"eval_twin": [], "eval_engine": [], "train_twin": [], "train_engine": []}
    for _ in range(3):
        rounds["eval_twin"].append(timed(lambda: twin.forward_infer(feat))["seconds"])
        rounds["eval_engine"].append(timed(lambda: eng.forward_infer(feat))["seconds"])
        rounds["train_twin"].append(timed(lambda: step(twin))["seconds"])
        rounds["train_engine"].append(timed(lambda: step(eng))["seconds"])
    for k, v in rounds.items():
        res[k] = {"seconds": sorted(v)[1], "rounds": v}
    res["eval_ratio_twin_over_engine"] = res["eval_twin"]["seconds"] / res["eval_engine"]["seconds"]
    res["train_ratio_twin_over_engine"] = res["train_twin"]["seconds"] / res["train_engine"]["seconds"]
    print("twin", json.dumps({k: v for k, v in res.items() if "ratio" in k or "diff" in k}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g2d_depthwise_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("g2d_depthwise_bench.py measures on the GPU; none is visible (nothing is measured elsewhere)")
    T._lib.get()
    dll = C.CDLL(T._lib.HIP_LIB_PATH)
    doc = {"what": "depthwise node of the 2-D graph engine on " + torch.cuda.get_device_name(0) + ": seconds per launch between device events (median of 5 "
                   "windows of >= 0.2 s after warm-up); bytes = x read + y written from the shapes; filter_gradient includes its chunk reduction",
           "shapes": {}}
    for name, c, h, w, k, s in (("dscnn_l_first_block", 276, 25, 10, (3, 3), (2, 2)), ("dscnn_l_block", 276, 13, 5, (3, 3), (1, 1)),
                                ("temporal_9x1", 64, 49, 1, (9, 1), (1, 1))):
        doc["shapes"][name] = bench_shape(dll, name, a.batch, c, h, w, k, s)
    doc["dscnn_l_twin"] = bench_twin(a.batch)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
