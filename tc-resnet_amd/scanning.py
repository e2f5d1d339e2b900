"""Offline keyword scanning of long recordings, on the device (tcr_scan of include/tcresnet_hip.h).

A `KeywordScanner` takes a batch of N signals of equal length and returns, for every signal and every step, exactly what a fresh
`streaming.StreamingDetector` with the same settings returns from its (i + 1)-th `push` when fed that signal k * hop samples at a
time: logits, probs, smoothed, top, score and is_new, bitwise.  One call computes every window at the network's batch throughput;
only the suppression rule runs in step order, over the candidate steps.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from ._lib import TcrError
from .engine import Frontend, TCResNet
from .streaming import _Detection

DEFAULT_MAX_WINDOWS = 4096


class ScanOutput(NamedTuple):
    """Results of a scan, on the device: logits / probs / smoothed [N, steps, classes] float32, top [N, steps] int32 (-1 before
    min_count steps), score [N, steps] float32, is_new [N, steps] int32 (1: a new detection of `top` at that step)."""
    logits: torch.Tensor
    probs: torch.Tensor
    smoothed: torch.Tensor
    top: torch.Tensor
    score: torch.Tensor
    is_new: torch.Tensor


class KeywordScanner(_Detection):
    """Scans signals through `frontend` and `net` with the streaming detector's settings (see `streaming.StreamingDetector`: the
    same arguments, the same ms -> steps conversion, the same weight and fold rules).  Step i of a signal is its window after
    (i + 1) * k * hop samples of audio, with one clip of silence in front.

    max_windows bounds the windows the network runs per launch (default 4096); the workspace, allocated once here, is sized by it
    and not by the signals' length."""

    def __init__(self, net: TCResNet, frontend: Frontend, frames_per_step: int = 1, average_window_ms: float = 1000,
                 min_count: int = 3, detection_threshold: float = 0.5, suppression_ms: float = 1500,
                 frozen_ss: Optional[torch.Tensor] = None, max_windows: Optional[int] = None):
        self._setup("KeywordScanner", "scanner", net, frontend, frames_per_step, average_window_ms, min_count, detection_threshold,
                    suppression_ms)
        self.max_windows = DEFAULT_MAX_WINDOWS if max_windows is None else int(max_windows)
        lib, cfg = self.lib, frontend.cfg
        nws = lib.tcr_scan_workspace_bytes(C.byref(cfg), net._h, self.k, self.max_windows)
        if nws == 0:
            raise TcrError(f"KeywordScanner: {lib.tcr_last_error().decode()}")
        self._bind_frozen(frozen_ss)
        self.workspace = torch.empty(nws // 4, dtype=torch.float32, device=self.device)

    def scan(self, samples: torch.Tensor) -> ScanOutput:
        """samples [N, L] float32 on the device, L a multiple of k * hop -> ScanOutput with L / (k * hop) steps per signal (new tensors).
        Refolds BN first when the net's weights changed (without `frozen_ss`); with `frozen_ss`, raises once the conv / fc arena
        changed since construction."""
        if samples.dim() != 2:
            raise TcrError(f"scan expects samples [N, L], got shape {tuple(samples.shape)}")
        self.net._check_tensor(samples, "scan samples")
        N, L = int(samples.shape[0]), int(samples.shape[1])        # (tcr_scan refuses N <= 0 and L not a multiple of k * hop)
        if self._frozen is not None:
            self._check_frozen_arena()
        ss = self._table()
        steps, ncls, dev = max(L // self.step_samples, 0), self.net.num_classes, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        out = ScanOutput(torch.empty((N, steps, ncls), **f32), torch.empty((N, steps, ncls), **f32), torch.empty((N, steps, ncls), **f32),
                         torch.empty((N, steps), **i32), torch.empty((N, steps), **f32), torch.empty((N, steps), **i32))
        fe, net = self.frontend, self.net
        self.lib.check(self.lib.tcr_scan(C.byref(fe.cfg), fe.plan.data_ptr(), net._h, net.params.data_ptr(), ss.data_ptr(), N, L, self.k,
                                         C.byref(self.det), samples.data_ptr(), self.workspace.data_ptr(), self.workspace.numel() * 4,
                                         *(t.data_ptr() for t in out), net._stream()), "tcr_scan")
        net._note_fold_reader()
        return out
