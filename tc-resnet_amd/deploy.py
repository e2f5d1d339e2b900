"""The deployable ("frozen") model: what the reference gets from build_deployable_model + freeze.py
(factory/audio_nets.py:87-125, freeze.py:16-49: a graph whose variables were converted to constants, fed either the raw
waveform `input/audio/before_preprocessing` [input_batch_size, samples, 1] through the DEPLOY-path MFCC, or features
`input` [1, height, width, channels]).

Here the artifact is the plan the fused eval kernel consumes directly -- no graph interpreter in between:
  * a JSON description (model name / scope / channels / input + output node names / front-end settings),
  * the constants: conv / fc weights under their TF variable names and, for TC-ResNet, every BatchNorm folded to a
    per-channel (scale, shift) table (tcr_net_fold_bn); DS-CNN keeps its variables and folds inside its eval kernel,
written as one `.npz` next to the checkpoint.  `FrozenModel.load(path)(x)` runs it on the HIP kernels.
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import runtime
from ._lib import HALO
from .engine import DSCNN, Frontend, Graph2D, TCResNet, features_to_planar

FORMAT = "tcresnet_amd.frozen/1"


@dataclass
class TensorSpec:
    """Stands in for the tf.placeholder / output tensor the reference's build_deployable_model returns."""
    name: str
    shape: Tuple[int, ...]
    dtype: str = "float32"

    @property
    def op(self):               # `output_tensor.op.name` is what freeze.py passes to convert_variables_to_constants
        return self


class FrozenModel:
    def __init__(self, meta: Dict, constants: Dict[str, np.ndarray], lib=None, device=None):
        if meta.get("format") != FORMAT:
            raise ValueError(f"not a {FORMAT} artifact")
        self.meta, self.constants = meta, constants
        lib = lib if lib is not None else runtime.default_lib()
        device = device if device is not None else runtime.default_device()
        fam = meta["family"]
        if fam == "tcresnet":
            self.engine = TCResNet(meta["scope"], meta["channels"], meta["width"], meta["height"], meta["num_classes"],
                                   bn_decay=meta["bn_decay"], bn_eps=meta["bn_eps"], lib=lib, device=device)
            self.engine.load_state_dict({k: v for k, v in constants.items() if k.endswith("/weights")}, strict=False)
            ss = np.ascontiguousarray(constants["__folded_batch_norm__"], dtype=np.float32).reshape(-1)
            full = int(self.engine.lib.tcr_net_frozen_floats(self.engine._h))
            if ss.size < full:      # the artifact stores scale / shift only: room for the weight image behind them
                ss = np.concatenate([ss, np.zeros(full - ss.size, np.float32)])
            self.frozen_ss = torch.from_numpy(ss).to(self.engine.device)
            # the conv weights are in `params` now and an artifact's never change: their fragment-ordered image, once (the table's flag set)
            self.engine.lib.check(self.engine.lib.tcr_net_fold_weights(self.engine._h, self.engine.params.data_ptr(), self.frozen_ss.data_ptr(),
                                                                       self.engine._stream()), "tcr_net_fold_weights")
        elif fam == "dscnn":
            self.engine = DSCNN(meta["size"], meta["height"], meta["width"], meta["num_classes"], lib=lib, device=device)
            self.engine.load_state_dict(constants)
            self.frozen_ss = None
        elif fam == "graph2d":
            import argparse
            from .factory import audio_nets
            saved = runtime.default_lib(), runtime.default_device()
            runtime.set_default(lib, device)
            try:
                model = getattr(audio_nets, meta["model"])(argparse.Namespace(**meta["args"]))
                self.engine = model._engine_for(torch.empty((1, meta["height"], meta["width"], 1)))
            finally:
                runtime.set_default(*saved)
            self.engine.load_state_dict(constants)
            self.frozen_ss = None
        else:
            raise ValueError(f"unknown model family {fam}")
        self.frontend: Optional[Frontend] = None
        if meta["include_preprocess"]:
            fe = meta["frontend"]
            self.frontend = Frontend(sample_rate=fe["sample_rate"], clip_duration_ms=fe["clip_duration_ms"],
                                     window_size_samples=fe["window_size_samples"], window_stride_samples=fe["window_stride_samples"],
                                     num_mel_bins=fe["num_mel_bins"], num_mfccs=fe["num_mfccs"], lower_edge_hertz=fe["lower_edge_hertz"],
                                     upper_edge_hertz=fe["upper_edge_hertz"], method=fe["method"], lib=lib, device=device)

    @property
    def input_tensors(self) -> List[TensorSpec]:
        return [TensorSpec(i["name"], tuple(i["shape"])) for i in self.meta["inputs"]]

    @property
    def output_tensor(self) -> TensorSpec:
        return TensorSpec(self.meta["output"]["name"], tuple(self.meta["output"]["shape"]))

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """x: waveforms [B, samples, 1] (include_preprocess) or features [B, height, width, channels]; returns softmax [B, classes]
        (the node named --output_name).  Any batch size runs; the reference's graph is fixed to input_batch_size."""
        if self.frontend is not None:
            planar = self.frontend(x if x.is_contiguous() else x.contiguous())
        else:
            planar = features_to_planar(x, lib=self.engine.lib)
        if self.frozen_ss is not None:
            return self.engine.forward_frozen(planar, self.frozen_ss)[1]
        return self.engine.forward_infer(planar)[1]

    def _detection_inputs(self, what: str):
        # (the front-end first: an artifact without one is refused before its engine is touched)
        if self.frontend is None:
            raise ValueError(f"{what} runs TC-ResNet, DS-CNN and 2-D graph artifacts exported with include_preprocess (this "
                             f"{self.meta['family']} artifact has none: it consumes features, the detector raw audio)")
        if self.meta["family"] not in ("tcresnet", "dscnn", "graph2d"):
            raise ValueError(f"{what} runs TC-ResNet, DS-CNN and 2-D graph artifacts (this one is {self.meta['family']})")
        return self.engine, self.frontend

    def streaming(self, n_streams: int, **kw):
        """A `streaming.StreamingDetector` of n_streams over this artifact (any family, exported with `include_preprocess`): the
        frozen front-end settings and the constants as exported (TC-ResNet: the conv / fc weights and the folded BN table; DS-CNN
        and 2-D graphs: every variable).  kw: frames_per_step, average_window_ms, min_count, detection_threshold, suppression_ms,
        max_windows (push_many's windows per network launch)."""
        net, fe = FrozenModel._detection_inputs(self, "streaming detection")
        from .streaming import StreamingDetector
        return StreamingDetector(net, fe, n_streams, frozen_ss=self.frozen_ss, **kw)

    def scanner(self, **kw):
        """A `scanning.KeywordScanner` over this artifact, like `streaming` (any family, exported with `include_preprocess`).  kw:
        frames_per_step, average_window_ms, min_count, detection_threshold, suppression_ms, max_windows."""
        net, fe = FrozenModel._detection_inputs(self, "keyword scanning")
        from .scanning import KeywordScanner
        return KeywordScanner(net, fe, frozen_ss=self.frozen_ss, **kw)

    def resampler(self, in_rate: int, n_streams: int, **kw):
        """A `resampling.Resampler` from in_rate to this artifact's sample rate (exported with `include_preprocess`), on the
        artifact's device: what turns recordings at another rate into the audio `streaming` / `scanner` take.  kw: dtype, channels,
        zero_crossings, beta, rolloff."""
        _, fe = FrozenModel._detection_inputs(self, "resampling to the model's rate")
        from .resampling import Resampler
        return Resampler(in_rate, int(fe.cfg.sample_rate), n_streams, device=fe.device, lib=fe.lib, **kw)

    # ---- file format ----------------------------------------------------------------------------------------------
    def save(self, path: str) -> str:
        out = {"__meta__": np.frombuffer(json.dumps(self.meta, sort_keys=True).encode(), dtype=np.uint8)}
        out.update(self.constants)
        with open(path, "wb") as fh:
            np.savez(fh, **out)
        return path

    @classmethod
    def load(cls, path: str, lib=None, device=None) -> "FrozenModel":
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(bytes(z["__meta__"]).decode())
            consts = {k: z[k] for k in z.files if k != "__meta__"}
        return cls(meta, consts, lib=lib, device=device)


def export_frozen(model, include_preprocess: bool, inputs: List[TensorSpec], output: TensorSpec) -> FrozenModel:
    """Variables -> constants for the model's current weights (graph_util.convert_variables_to_constants)."""
    eng, args = model.engine, model.args
    sd = eng.state_dict()
    meta = {"format": FORMAT, "model": type(model).__name__, "num_classes": int(args.num_classes), "include_preprocess": bool(include_preprocess),
            "inputs": [{"name": i.name, "shape": list(i.shape)} for i in inputs], "output": {"name": output.name, "shape": list(output.shape)},
            "height": int(args.height), "width": int(args.width), "channels": int(args.channels)}
    if isinstance(eng, TCResNet):
        meta.update(family="tcresnet", scope=eng.scope, channels=[int(c) for c in eng.channels], bn_decay=float(eng.cfg.bn_decay),
                    bn_eps=float(eng.cfg.bn_eps))
        consts = {k: v for k, v in sd.items() if k.endswith("/weights")}
        consts["__folded_batch_norm__"] = eng.fold_bn()[:eng.n_stat].cpu().numpy()        # scale / shift only (2 x c_pad per BN unit, as the moving statistics): the loader rebuilds the weight image
    elif isinstance(eng, DSCNN):
        meta.update(family="dscnn", size=eng.size)
        consts = dict(sd)
    elif isinstance(eng, Graph2D):
        meta.update(family="graph2d", args={k: v for k, v in vars(args).items() if isinstance(v, (int, float, str, bool)) or v is None})
        consts = dict(sd)
    else:
        raise NotImplementedError(f"frozen export of {type(eng).__name__}")
    if include_preprocess:
        fe = model._preprocessor._frontend
        meta["frontend"] = {"sample_rate": int(fe.cfg.sample_rate), "clip_duration_ms": int(fe.cfg.n_samples * 1000 // fe.cfg.sample_rate),
                            "window_size_samples": int(fe.cfg.win), "window_stride_samples": int(fe.cfg.hop), "num_mel_bins": int(fe.cfg.n_mel),
                            "num_mfccs": int(fe.cfg.n_coef), "lower_edge_hertz": float(fe.cfg.lower_hz), "upper_edge_hertz": float(fe.cfg.upper_hz),
                            "method": {0: "mfcc", 1: "log_mel_spectrogram", 2: "mfcc_deploy"}[int(fe.cfg.method)]}
    return FrozenModel(meta, consts, lib=eng.lib, device=eng.device)
