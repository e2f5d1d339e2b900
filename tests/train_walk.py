"""Teacher-forced training walks (tests/test_train_walk.py): many optimisation steps on the kernels, each step compared with the
float64 oracle's step FROM THE STATE THE KERNELS HOLD at that step (parameters, moving statistics, optimiser slots read back).

Why teacher-forced: two faithful implementations that run free separate as soon as one ReLU input changes side (float32 torch
against the float64 oracle on TCResNet8-1.0, same batches: parameters 2.5e-6 apart for 60 steps at batch 24, 9.5e-3 apart after
40 steps at batch 5, 8e-2 after 4 steps on TCResNet14-1.5).  Started from the kernels' own state, every step is as tight as the
one-step checks of tests/common.py -- and sees what those never see: non-zero slots on trained weights, moving statistics away
from their initial values, the learning rate behind a boundary, Adam's t above 3, an advanced dropout stream, a workspace reused
across batch sizes, an eval forward whose BN fold has to be refreshed after an optimiser step.

Three roles, so that the SAME comparison code runs on the kernels and on the oracle-side controls:
  subject   what is stepped and read back: the kernels (KernelSubject) or a float32 torch restatement (TorchSubject)
  oracle    float64 forward / backward / optimiser formulas / expectations of one net family; a perturbed copy overrides one method
  Schedule  what drives the subject: optimiser, learning rate and batch size per step
"""
import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional

import numpy as np
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from oracle import torch_ref as TR
from oracle.make_golden import dropout_mask
from tests import common as Cm
from tests.test_net_configs import GRAD_RTOL, OPT_TOL, PROB_TOL, STAT_TOL, STEP_TOL

MARGIN_MIN = 1e-6           # tests/common.py::check_small_batch's bound on the oracle's closest ReLU input
LOSS_TOL, L2_TOL = 1e-4, 1e-5       # tests/common.py::check_train's bounds on the model loss and the L2 term
# The step size recovered from the read-back values over the entries with |dw| >= MOVED * |w|: w' = fl(w - step) is half an ulp of
# w (6e-8 |w|) off, i.e. at most 6e-5 of such a dw; the median over thousands of entries is far inside 1e-3.  1e-3 separates 0.1
# from 0.01 and Adam's t from t +- 1 from step 10 on (0.5 % at t = 10, 1.2 % at t = 24).
LR_RTOL, MOVED = 1e-3, 1e-3
SLOTS = {"mom": ("Momentum",), "adam": ("Adam", "Adam_1"), "rmsprop": ("RMSProp", "RMSProp_1")}
EMA = "ExponentialMovingAverage"


@dataclass
class Schedule:
    opt: str                                    # "mom" | "adam" | "rmsprop"
    lr: Callable[[int], float]                  # 0-based step (the trainer's global_step before the step) -> learning rate
    hp: Dict[str, float]                        # mom: mu; adam: b1, b2, eps; rmsprop: decay, momentum, eps
    batch: Callable[[int], int]
    wd: float = 1e-3
    keep_prob: float = 0.5
    ema: Optional[float] = None                 # decay of the shadow variables stepped behind every optimiser step


def momentum_schedule(boundaries, values, batch, mu=0.9, wd=1e-3):
    return Schedule("mom", lambda t: R.piecewise_constant_lr(t, list(boundaries), list(values)), {"mu": mu}, batch, wd)


def adam_schedule(lr, batch, wd=1e-3):
    return Schedule("adam", lambda t: lr, {"b1": 0.9, "b2": 0.999, "eps": 1e-8}, batch, wd)


def rmsprop_schedule(lr, batch, decay=0.8, momentum=0.5, eps=1e-3, wd=1e-3, ema=0.9):
    return Schedule("rmsprop", lambda t: lr, {"decay": decay, "momentum": momentum, "eps": eps}, batch, wd, ema=ema)


# ---- float64 optimiser formulas (tf.train.*Optimizer as csrc/optim.hip states them) ---------------------------------------------------
def adam_factor(hp, t1):
    return math.sqrt(1.0 - hp["b2"] ** t1) / (1.0 - hp["b1"] ** t1)


def opt_step64(opt, hp, lr, t1, w, gv, slots):
    """One tensor: (w', slots') from w, the regularised gradient gv and the slots {slot name: array}.  t1: Adam's 1-based t."""
    if opt == "mom":
        a = hp["mu"] * slots["Momentum"] + gv
        return w - lr * a, {"Momentum": a}
    if opt == "adam":
        m = slots["Adam"] + (1.0 - hp["b1"]) * (gv - slots["Adam"])
        v = slots["Adam_1"] + (1.0 - hp["b2"]) * (gv * gv - slots["Adam_1"])
        return w - lr * adam_factor(hp, t1) * m / (np.sqrt(v) + hp["eps"]), {"Adam": m, "Adam_1": v}
    if opt == "rmsprop":
        ms = slots["RMSProp"] + (1.0 - hp["decay"]) * (gv * gv - slots["RMSProp"])
        mo = hp["momentum"] * slots["RMSProp_1"] + lr * gv / np.sqrt(ms + hp["eps"])
        return w - mo, {"RMSProp": ms, "RMSProp_1": mo}
    raise ValueError(opt)


def _flat(d, names):
    return np.concatenate([np.asarray(d[k], np.float64).ravel() for k in names])


def applied_step(opt, hp, names, p0, p1, gv, slots0, slots1):
    """The step size the subject APPLIED, recovered from what was read back (median over the entries that moved by >= MOVED |w|):
    momentum  -dw / accum'                       = lr
    adam      -dw (sqrt(v') + eps) / m'          = lr sqrt(1 - b2^t) / (1 - b1^t)
    rmsprop   (mom' - momentum mom) sqrt(ms' + eps) / g = lr, and -dw / mom' = 1 (returned second)."""
    w0, w1 = _flat(p0, names), _flat(p1, names)
    dw = w1 - w0
    sel = (np.abs(dw) >= MOVED * np.abs(w0)) & (dw != 0)
    assert sel.sum() >= 100, ("too few entries moved to recover a step size", int(sel.sum()))
    s1 = {n: _flat(slots1[n], names) for n in SLOTS[opt]}
    with np.errstate(divide="ignore", invalid="ignore"):
        if opt == "mom":
            return float(np.median((-dw / s1["Momentum"])[sel])), 1.0
        if opt == "adam":
            return float(np.median((-dw * (np.sqrt(s1["Adam_1"]) + hp["eps"]) / s1["Adam"])[sel])), 1.0
        g = _flat(gv, names)
        sel &= np.abs(g) > 1e-3 * np.abs(g).max()
        mo0 = _flat(slots0["RMSProp_1"], names)
        lr = (s1["RMSProp_1"] - hp["momentum"] * mo0) * np.sqrt(s1["RMSProp"] + hp["eps"]) / g
        return float(np.median(lr[sel])), float(np.median((-dw / s1["RMSProp_1"])[sel]))


# ---- oracles ---------------------------------------------------------------------------------------------------------------------
class Oracle:
    """What one net family's float64 side provides to walk().  The expectation methods (lr, opt_t, seed, update, new_stats, eval) are
    what a perturbed copy overrides: each restates ONE thing the subject is expected to do."""
    grad_rtol = GRAD_RTOL
    margin_min = MARGIN_MIN

    def __init__(self, sched: Schedule):
        self.sched = sched

    # expectations ------------------------------------------------------------------------------------------------------------
    def lr(self, t0):
        return self.sched.lr(t0)

    def opt_t(self, t0):
        return t0 + 1

    def seed(self, t0):
        return t0

    def decays(self, name):
        return R.is_l2_param(name)

    def exact_zero(self, name):
        return False

    def regularised(self, p, g):
        return {k: g[k] + (self.sched.wd * p[k] if self.decays(k) else 0.0) for k in g}

    def update(self, p, g, slots, t0):
        """Float64 optimiser step on the (unregularised) gradient g from the read-back parameters and slots."""
        gv = self.regularised(p, g)
        p1, s1 = {}, {n: {} for n in SLOTS[self.sched.opt]}
        for k in g:
            p1[k], sl = opt_step64(self.sched.opt, self.sched.hp, self.lr(t0), self.opt_t(t0), p[k], gv[k], {n: slots[n][k] for n in s1})
            for n in s1:
                s1[n][k] = sl[n]
        return p1, s1

    def expected_step(self, t0):
        return self.lr(t0) * (adam_factor(self.sched.hp, self.opt_t(t0)) if self.sched.opt == "adam" else 1.0)

    def new_stats(self, s, rec, t0):
        return rec["new_stats"]

    def eval_state(self, p, s):
        return p, s

    # the family ----------------------------------------------------------------------------------------------------------------
    def make_batch(self, b, t0, k):
        raise NotImplementedError

    def forward(self, p, s, batch, t0):
        """Train-mode forward: dict(logits, loss, l2, new_stats, margin, ...)."""
        raise NotImplementedError

    def backward(self, p, rec, batch):
        """Gradients of the MODEL loss (the regulariser enters through `regularised`)."""
        raise NotImplementedError

    def eval(self, p, s, batch):
        raise NotImplementedError


class TCOracle(Oracle):
    """TC-ResNet on waveforms: oracle/numpy_ref.py behind its own float64 MFCC."""

    def __init__(self, sched, name="TCResNet8", width=1.0, tag="4020", base_seed=5000):
        super().__init__(sched)
        self.name, self.width, self.tag = name, width, tag
        self.cfg = R.FRONTEND_4020 if tag == "4020" else R.FRONTEND_3010
        self.arch = R.make_tcresnet(name, float(width))
        self.last_channels = R.tcresnet_channels(name, float(width))[-1]
        self.base_seed = base_seed
        self.seed_offset = 0            # the trainer seeds step t0 (0-based) with its 1-based step count: seed_offset = 1

    def seed(self, t0):
        return t0 + self.seed_offset

    def init_state(self, seed=5):
        p, s = R.init_params(self.arch, seed)
        return ({k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}, {k: v.astype(np.float32).astype(np.float64) for k, v in s.items()})

    def make_batch(self, b, t0, k):
        wav = R.synth_waveforms(b, seed=self.base_seed + t0, start=b * k)
        return {"wav": wav, "x": R.mfcc(wav, self.cfg), "labels": R.synth_labels(b, start=t0 + 5 * k).astype(np.float64)}

    def batch_of(self, wav, labels):
        return {"wav": np.asarray(wav, np.float32), "x": R.mfcc(np.asarray(wav, np.float32), self.cfg), "labels": np.asarray(labels, np.float64)}

    def forward(self, p, s, batch, t0):
        b, keep = batch["x"].shape[0], self.sched.keep_prob
        mask = dropout_mask(self.seed(t0), 0, b, self.last_channels, keep) if keep < 1.0 else None
        with np.errstate(over="ignore"):        # (the `ranges` sigmoid of a trained net's large pre-activations)
            f = R.forward(self.arch, p, s, batch["x"], True, keep, mask)
        _, model, l2 = R.loss(f["logits"], batch["labels"], p, self.sched.wd)
        return {"logits": f["logits"], "loss": model, "l2": l2, "new_stats": f["new_stats"], "margin": Cm.relu_margin(self.arch, f), "fwd": f}

    def backward(self, p, rec, batch):
        return R.backward(self.arch, p, rec["fwd"], batch["labels"], 0.0)

    def eval(self, p, s, batch):
        with np.errstate(over="ignore"):
            f = R.forward(self.arch, p, s, batch["x"], False)
        return f["logits"], f["probs"]


class DSOracle(Oracle):
    """DS-CNN on waveforms (10 coefficients): oracle/dscnn_ref.py.  No dropout in the graph; every trainable is decayed (the reference's
    name filter excludes "BatchNorm", these scopes are "batch_norm"); a bias ahead of a train-mode BN has gradient zero.
    margin_min: tests/common.py::check_dscnn_train_live's 2e-6 -- 430 000 BN outputs feed a ReLU at batch 6, and on the MI355X ONE input that
    the oracle has at +1.83e-6 (the best of six candidates at that step) came out on the other side in float32: that unit's filter gradient
    moved by 1.3 %, every other step of the walk stayed within 5e-6.  With that check's 12 candidates the best margin stays at or above 3.3e-6."""
    margin_min = 2e-6

    def __init__(self, sched, size="S", base_seed=6000):
        import dataclasses
        from oracle import dscnn_ref as D
        super().__init__(sched)
        self.D, self.size, self.blocks = D, size, D.net_def(size)
        self.cfg = dataclasses.replace(R.FRONTEND_4020, num_mfccs=10)
        self.base_seed = base_seed

    def init_state(self, seed=3):
        p, s = self.D.init_params(self.blocks, seed=seed, randomize=False)
        return ({k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}, {k: v.astype(np.float32).astype(np.float64) for k, v in s.items()})

    def decays(self, name):
        return True

    def exact_zero(self, name):
        return name.endswith("/biases") and "fc1" not in name

    make_batch = TCOracle.make_batch

    def forward(self, p, s, batch, t0):
        D = self.D
        f = D.forward(self.blocks, p, s, batch["x"], True)
        margin = min(float(np.abs(c["xhat"] + p[k + "/beta"]).min()) for k, c in f["cache"].items() if isinstance(c, dict))
        l2 = self.sched.wd * sum(0.5 * float((v ** 2).sum()) for v in p.values())
        return {"logits": f["logits"], "loss": D.loss(f["logits"], batch["labels"]), "l2": l2, "new_stats": f["new_stats"], "margin": margin, "fwd": f}

    def backward(self, p, rec, batch):
        return self.D.backward(self.blocks, p, rec["fwd"], batch["labels"])

    def eval(self, p, s, batch):
        f = self.D.forward(self.blocks, p, s, batch["x"], False)
        return f["logits"], f["probs"]


class G2DOracle(Oracle):
    """A Res* graph model on feature planes: oracle/net2d_ref.py (autograd).  `margin`: the closest ReLU input of the train-mode forward."""

    def __init__(self, sched, variant, t, f, decays, grad_rtol, base_seed=7000):
        from oracle import net2d_ref as O
        super().__init__(sched)
        self.O, self.variant, self.t, self.f, self._decays, self.grad_rtol, self.base_seed = O, variant, t, f, set(decays), grad_rtol, base_seed

    def decays(self, name):
        return name in self._decays

    def make_batch(self, b, t0, k):
        x = np.random.RandomState(self.base_seed + 16 * t0 + k).uniform(-2.0, 2.0, (b, self.t, self.f)).astype(np.float32)
        return {"feat": x, "x": x.astype(np.float64), "labels": R.synth_labels(b, start=t0 + 5 * k).astype(np.float64)}

    def forward(self, p, s, batch, t0):
        O = self.O
        st = {k: torch.tensor(v) for k, v in s.items()}
        xt = torch.tensor(batch["x"])
        O.KINK_LOG.update(on=True, near=0, total=0, decide=None, idx=0, followed=0, min=float("inf"))
        try:
            out, model, _, grads = O.loss_and_grads(lambda pp: O.res_forward(pp, st, xt, self.variant, True), p, batch["labels"])
        finally:
            O.KINK_LOG.update(on=False)
        l2 = self.sched.wd * sum(0.5 * float((v ** 2).sum()) for k, v in p.items() if self.decays(k))
        return {"logits": out["logits"], "loss": model, "l2": l2, "new_stats": out["new_stats"], "margin": O.KINK_LOG["min"], "grads": grads}

    def backward(self, p, rec, batch):
        return rec["grads"]

    def eval(self, p, s, batch):
        with torch.no_grad():
            out = self.O.res_forward({k: torch.tensor(v) for k, v in p.items()}, {k: torch.tensor(v) for k, v in s.items()},
                                     torch.tensor(batch["x"]), self.variant, False)
        return out["logits"].numpy(), out["probs"].numpy()


# ---- subjects --------------------------------------------------------------------------------------------------------------------
class KernelSubject:
    """An engine object (TCResNet / DSCNN / Graph2D) stepped through its kernels and read back in the oracle's shapes."""

    def __init__(self, lib, net, state, sched, frontend=None, waveform_paths=False, held_out=None):
        self.lib, self.net, self.sched, self.fe = lib, net, sched, frontend
        p, s = state
        self.shapes = {k: v.shape for k, v in list(p.items()) + list(s.items())}
        self.names, self.stat_names = list(p), list(s)
        sd = dict(p)
        sd.update(s)
        net.load_state_dict(sd)
        net.slots.clear()
        for n in SLOTS[sched.opt]:
            net.slot_arena(n)
        if sched.ema is not None:
            net.ema_init()
        self.call = None
        if waveform_paths:          # a prepared call bound BEFORE the walk: it must refuse (engine.py::waveform_call) or be fresh, never stale
            self.held_wav = Cm.to_dev(lib, held_out["wav"])
            b = self.held_wav.shape[0]
            self.call_out = (torch.zeros((b, net.num_classes), dtype=torch.float32, device=net.device), torch.zeros((b, net.num_classes), dtype=torch.float32, device=net.device))
            self.call = net.waveform_call(frontend, self.held_wav, self.call_out)

    def _arena_dict(self, arena, names):
        a = arena.detach().cpu().numpy().astype(np.float64)
        return {k: a[self.net.tensors[k].offset:self.net.tensors[k].offset + self.net.tensors[k].size].reshape(self.shapes[k]) for k in names}

    def read(self):
        net = self.net
        slots = {n: self._arena_dict(net.slots[n], self.names) for n in SLOTS[self.sched.opt]}
        if self.sched.ema is not None:
            slots[EMA] = self._arena_dict(net.slots[EMA], self.names)
        return self._arena_dict(net.params, self.names), self._arena_dict(net.stats, self.stat_names), slots

    def features(self, batch):
        if self.fe is not None:
            return self.fe(Cm.to_dev(self.lib, batch["wav"]))
        return T.features_to_planar(torch.from_numpy(np.ascontiguousarray(batch["feat"], dtype=np.float32)).to(self.net.device), lib=self.lib)

    def train(self, batch, t0, lr):
        net, sc = self.net, self.sched
        b = batch["labels"].shape[0]
        logits, _, loss_sum = net.forward_train(self.features(batch), Cm.to_dev(self.lib, batch["labels"]), keep_prob=sc.keep_prob, seed=t0, sample_offset=0)
        net.backward()
        out = {"logits": logits.cpu().numpy().astype(np.float64), "loss": float(loss_sum) / b, "l2": float(net.l2_loss(sc.wd)),
               "grads": self._arena_dict(net.grads, self.names)}
        if sc.opt == "mom":
            net.sgd_momentum_step(lr, sc.hp["mu"], sc.wd)
        elif sc.opt == "adam":
            net.adam_step(lr, t0 + 1, sc.hp["b1"], sc.hp["b2"], sc.hp["eps"], weight_decay=sc.wd)
        else:
            net.rmsprop_step(lr, sc.hp["decay"], sc.hp["momentum"], sc.hp["eps"], weight_decay=sc.wd)
        if sc.ema is not None:
            net.ema_step(sc.ema)
        return out

    def evals(self, batch):
        """{path: (logits, probs) | "refused"} of the eval paths on `batch`."""
        net = self.net
        lg, pr = net.forward_infer(self.features(batch))
        out = {"forward_infer": (lg.cpu().numpy(), pr.cpu().numpy())}
        if self.call is not None:
            lg, pr = net.forward_waveform(self.fe, Cm.to_dev(self.lib, batch["wav"]))
            out["forward_waveform"] = (lg.cpu().numpy(), pr.cpu().numpy())
            out["waveform_call"] = self.run_call(self.call, self.call_out)
            # ... and one prepared now, on the weights as they are, must run
            fresh_out = (torch.zeros_like(self.call_out[0]), torch.zeros_like(self.call_out[1]))
            out["waveform_call_fresh"] = self.run_call(net.waveform_call(self.fe, self.held_wav, fresh_out), fresh_out)
        return out

    @staticmethod
    def run_call(call, outs):
        outs[0].zero_(); outs[1].zero_()
        try:
            call()
        except T.TcrError:
            return "refused"
        return outs[0].cpu().numpy(), outs[1].cpu().numpy()


class TorchSubject:
    """The float32 torch counterpart of TCOracle (oracle/torch_ref.py with autograd, the optimiser formulas in float32): the clean
    partner of the oracle-side controls, and (float32_loss_ratio) the float32 yardstick of the convergence test's loss bound.
    seed_offset: added to the step for the dropout seed (the trainer seeds with its 1-based step count)."""

    def __init__(self, oracle: TCOracle, state, sched, seed_offset=0):
        self.o, self.sched, self.seed_offset = oracle, sched, seed_offset
        p, s = state
        self.names, self.stat_names = list(p), list(s)
        self.p = {k: torch.tensor(v, dtype=torch.float32) for k, v in p.items()}
        self.s = {k: torch.tensor(v, dtype=torch.float32) for k, v in s.items()}
        init = {"RMSProp": torch.ones_like}
        self.slots = {n: {k: init.get(n, torch.zeros_like)(v) for k, v in self.p.items()} for n in SLOTS[sched.opt]}

    def read(self):
        n64 = lambda d: {k: v.numpy().astype(np.float64) for k, v in d.items()}
        return n64(self.p), n64(self.s), {n: n64(d) for n, d in self.slots.items()}

    def train(self, batch, t0, lr):
        sc, o = self.sched, self.o
        b = batch["labels"].shape[0]
        params = {k: v.detach().requires_grad_(True) for k, v in self.p.items()}
        mask = torch.tensor(dropout_mask(t0 + self.seed_offset, 0, b, o.last_channels, sc.keep_prob), dtype=torch.float32) if sc.keep_prob < 1.0 else None
        f = TR.forward(o.arch, params, self.s, torch.tensor(batch["x"], dtype=torch.float32), True, sc.keep_prob, mask)
        tot, model = TR.total_loss(f["logits"], torch.tensor(batch["labels"], dtype=torch.float32), params, sc.wd)
        model.backward()
        grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in params.items()}
        out = {"logits": f["logits"].detach().numpy().astype(np.float64), "loss": float(model.detach()), "l2": float((tot - model).detach()),
               "grads": {k: g.numpy().astype(np.float64) for k, g in grads.items()}}
        f32 = np.float32
        with torch.no_grad():
            for k, w in self.p.items():
                gv = grads[k] + (f32(sc.wd) * w if o.decays(k) else 0.0)
                if sc.opt == "mom":
                    a = self.slots["Momentum"][k] = f32(sc.hp["mu"]) * self.slots["Momentum"][k] + gv
                    self.p[k] = w - f32(lr) * a
                elif sc.opt == "adam":
                    m = self.slots["Adam"][k] = self.slots["Adam"][k] + f32(1.0 - sc.hp["b1"]) * (gv - self.slots["Adam"][k])
                    v = self.slots["Adam_1"][k] = self.slots["Adam_1"][k] + f32(1.0 - sc.hp["b2"]) * (gv * gv - self.slots["Adam_1"][k])
                    self.p[k] = w - f32(lr * adam_factor(sc.hp, t0 + 1)) * m / (torch.sqrt(v) + f32(sc.hp["eps"]))
                else:
                    raise ValueError(sc.opt)
            self.s = {k: v.detach() for k, v in f["new_stats"].items()}
        return out

    def evals(self, batch):
        with torch.no_grad():
            f = TR.forward(self.o.arch, self.p, self.s, torch.tensor(batch["x"], dtype=torch.float32), False)
        return {"forward_infer": (f["logits"].numpy(), f["probs"].numpy())}


# ---- the walk --------------------------------------------------------------------------------------------------------------------
class Worst:
    """Per quantity: the worst error, its tolerance and the step it was seen at; `ratio(q)` = worst error / tolerance."""

    def __init__(self, check):
        self.check, self.rows, self.min_margin, self.max_eval_logit = check, {}, float("inf"), 0.0

    def see(self, q, err, tol, t0, what=""):
        err = float(err)
        if q not in self.rows or err / tol > self.rows[q][0] / self.rows[q][1]:
            self.rows[q] = (err, tol, t0)
        if self.check:
            assert err < tol, f"step {t0}: {q} {what}: error {err:.3e} >= {tol:.3e}"

    def ratio(self, q):
        return self.rows[q][0] / self.rows[q][1] if q in self.rows else 0.0

    def table(self, title):
        lines = [f"{title}: smallest ReLU margin {self.min_margin:.2e}, largest eval logit {self.max_eval_logit:.3g}"]
        lines += [f"  {q:<16} worst {e:.3e}  (bound {tol:.1e}, step {t0})" for q, (e, tol, t0) in self.rows.items()]
        return "\n".join(lines)


def _same_state(a, b):
    return all(np.array_equal(x[k], y[k]) for x, y in zip(a[:2], b[:2]) for k in x) and \
        all(np.array_equal(a[2][n][k], b[2][n][k]) for n in a[2] for k in a[2][n])


# Eval logits of a net a few steps into training are LARGE: the moving statistics (decay 0.997) have moved 2 % of the way to the batch
# statistics the weights were trained under, so eval-mode BN barely normalises -- logits reach 1e3 to 1.5e4 where the fixtures' reach
# 20, and LOGIT_TOL = 1e-4 absolute is then below float32 resolution (one ulp of 15 000 is 1e-3).  Measured at such states (TCResNet8-1.0,
# momentum walk, every fourth step): the float32 torch oracle is 1.9e-7 to 4.5e-7 of the largest logit from the float64 oracle, the
# kernels 1.4e-7 to 4.1e-7.  Bound: LOGIT_TOL up to a largest logit of 50, above that 2e-6 of the largest logit (4.4 x the float32 torch
# oracle's worst, 17 ulps).  The probabilities keep PROB_TOL: a softmax over logits that far apart is saturated.
EVAL_REL = 2e-6


def eval_scale(ref_logits):
    return max(1.0, EVAL_REL * float(np.abs(ref_logits).max()) / Cm.LOGIT_TOL)


def compare_eval(w, oracle, subject, p, s, held, t0, tag=""):
    """The subject's eval paths on the held-out batch against the oracle's eval forward from the read-back state."""
    ref_l, ref_p = oracle.eval(*oracle.eval_state(p, s), held)
    scale = eval_scale(ref_l)
    w.max_eval_logit = max(w.max_eval_logit, float(np.abs(ref_l).max()))
    for path, got in subject.evals(held).items():
        if isinstance(got, str):        # a prepared call that refuses to run on changed weights: what engine.py documents
            assert got == "refused" and path == "waveform_call", (path, got)
            continue
        w.see(tag + "eval_logits", np.abs(got[0] - ref_l).max(), Cm.LOGIT_TOL * scale, t0, path)
        w.see(tag + "eval_probs", np.abs(got[1] - ref_p).max(), PROB_TOL, t0, path)
        if w.check:
            assert np.array_equal(got[0].argmax(1), ref_l.argmax(1)), f"step {t0}: {path}: argmax differs"


def walk(subject, oracle, sched, steps, held, k_cands=3, eval_every=4, check=True, title="walk"):
    """Teacher-forced walk of `steps` optimisation steps; returns the Worst table (check=False: nothing asserted but the inputs'
    conditioning -- the controls read the ratios)."""
    w = Worst(check)
    names = subject.names
    state = subject.read()
    for t0 in range(steps):
        p, s, slots = state
        b = sched.batch(t0)
        # the batch, of k_cands candidates, whose train-mode ReLU inputs stay farthest from zero under the oracle AT THIS STATE
        best = None
        for k in range(k_cands):
            cand = oracle.make_batch(b, t0, k)
            rec = oracle.forward(p, s, cand, t0)
            if best is None or rec["margin"] > best[1]["margin"]:
                best = (cand, rec)
        batch, rec = best
        assert rec["margin"] > oracle.margin_min, f"step {t0}: ReLU margin {rec['margin']:.2e} of the best of {k_cands} candidate batches"
        w.min_margin = min(w.min_margin, rec["margin"])
        gref = oracle.backward(p, rec, batch)
        lr = sched.lr(t0)
        got = subject.train(batch, t0, lr)
        state = p1, s1, slots1 = subject.read()
        # forward, loss, gradients, moving statistics
        w.see("train_logits", np.abs(got["logits"] - rec["logits"]).max(), Cm.LOGIT_TOL, t0)
        w.see("model_loss", abs(got["loss"] - rec["loss"]), LOSS_TOL, t0)
        w.see("l2_loss", abs(got["l2"] - rec["l2"]), L2_TOL, t0)
        for k in names:
            if oracle.exact_zero(k):
                assert np.abs(gref[k]).max() < 1e-10 and np.all(got["grads"][k] == 0.0), f"step {t0}: {k}: gradient of a bias ahead of a train-mode BN"
                continue
            w.see("grads", np.abs(got["grads"][k] - gref[k]).max() / max(np.abs(gref[k]).max(), 1e-3), oracle.grad_rtol, t0, k)
        for k, ref in oracle.new_stats(s, rec, t0).items():
            w.see("moving_stats", np.abs(s1[k] - ref).max() / max(1.0, np.abs(ref).max()), STAT_TOL, t0, k)
        # the optimiser: from the subject's OWN gradient and the read-back slots (a ReLU-sign difference cannot enter; Adam's first
        # steps are a function of the gradient's sign) ...
        pw, sw = oracle.update(p, got["grads"], slots, t0)
        for k in names:
            w.see("opt_params", np.abs(p1[k] - pw[k]).max(), OPT_TOL, t0, k)
            for n in sw:
                w.see("opt_slots", np.abs(slots1[n][k] - sw[n][k]).max(), OPT_TOL, t0, f"{k}/{n}")
        # ... for momentum also from the oracle's gradient (the bound of one step at lr 0.1, scaled with the step size)
        if sched.opt == "mom":
            pr, _ = oracle.update(p, {k: (got["grads"][k] if oracle.exact_zero(k) else gref[k]) for k in names}, slots, t0)
            for k in names:
                w.see("step_params", np.abs(p1[k] - pr[k]).max(), STEP_TOL * oracle.lr(t0) / 0.1, t0, k)
        # the step size that was applied
        step, unit = applied_step(sched.opt, sched.hp, names, p, p1, oracle.regularised(p, got["grads"]), slots, slots1)
        want = oracle.expected_step(t0)
        w.see("step_size_rel", abs(step / want - 1.0), LR_RTOL, t0, f"applied {step:.6g}, schedule {want:.6g}")
        if sched.opt == "rmsprop":
            w.see("step_is_slot_rel", abs(unit - 1.0), LR_RTOL, t0)
        if sched.ema is not None:
            for k in names:
                want_sh = slots[EMA][k] - (1.0 - sched.ema) * (slots[EMA][k] - p1[k])
                w.see("ema_shadow", np.abs(slots1[EMA][k] - want_sh).max(), OPT_TOL, t0, k)
        # the eval paths, whose BN fold has to follow the step
        if (t0 + 1) % eval_every == 0 or t0 == steps - 1:
            compare_eval(w, oracle, subject, p1, s1, held, t0)
            # nothing the eval paths do may touch what the next step starts from
            assert _same_state(state, subject.read()), f"step {t0}: an eval forward changed the variables, statistics or slots"
    print(w.table(f"{title} ({steps} steps, K = {k_cands})"))
    return w


# ---- free-running training (the convergence test) ---------------------------------------------------------------------------------
WORDS = ["down", "go", "left", "no", "off", "on", "right", "stop", "unknown", "up", "yes"]      # + __null__ (silent samples) = 12 classes


def write_wav(path, pcm, rate=16000):
    import struct
    pcm = np.asarray(pcm, dtype="<i2")
    body = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, rate * 2, 2, 16) + b"data" + struct.pack("<I", pcm.nbytes) + pcm.tobytes()
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)


def write_tone_dataset(root, per_class, seed=0):
    """A learnable WAV directory (<root>/<split>/<label>/*.wav): a clip of class c is 0.3 uniform noise + 0.25 sin(2 pi (300 + 250 c) t + phi)
    + 0.15 sin(2 pi (3500 - 200 c) t), one second of 16-bit PCM; c = the label's index (0 is __null__: the silent samples of --num_silent).
    per_class = {split: clips per word}; the splits draw different noise and phases."""
    rng = np.random.RandomState(seed)
    t = np.arange(16000) / 16000.0
    for split, n in per_class.items():
        for c, word in enumerate(WORDS, start=1):
            d = root / split / word
            d.mkdir(parents=True)
            for g in range(n):
                x = 0.3 * rng.uniform(-1.0, 1.0, 16000) + 0.25 * np.sin(2 * np.pi * (300 + 250 * c) * t + rng.uniform(0, 2 * np.pi)) \
                    + 0.15 * np.sin(2 * np.pi * (3500 - 200 * c) * t)
                write_wav(d / f"{g:03d}.wav", np.round(x * 32767.0))


def dataset_batches(ds, steps):
    """The first `steps` batches of a dataset object, from its start, as oracle batches (float64 MFCC is the caller's)."""
    ds.setup_iterator()
    out = []
    for _ in range(steps):
        wav, labels = ds.next_batch()
        out.append((wav[..., 0].cpu().numpy(), labels.cpu().numpy().astype(np.float64)))
    ds.setup_iterator()
    return out


def free_run_oracle(oracle, state, batches):
    """The float64 oracle trained on `batches` with oracle.sched from `state`: (per-step model loss, final (p, s))."""
    p, s = state
    init = {"RMSProp": np.ones_like}
    slots = {n: {k: init.get(n, np.zeros_like)(v) for k, v in p.items()} for n in SLOTS[oracle.sched.opt]}
    losses = []
    for t0, batch in enumerate(batches):
        rec = oracle.forward(p, s, batch, t0)
        p, slots = oracle.update(p, oracle.backward(p, rec, batch), slots, t0)
        s = rec["new_stats"]
        losses.append(rec["loss"])
    return np.asarray(losses), (p, s)


def block_means(losses, blocks=6):
    losses = np.asarray(losses, np.float64)
    assert len(losses) % blocks == 0
    return losses.reshape(blocks, -1).mean(axis=1)


def float32_loss_ratio(oracle, state, batches):
    """Mean model loss over the last sixth of a free run on `batches`: the float32 torch oracle's over the float64 oracle's (same
    initialisation, batches and dropout masks).  What the convergence test's bound on the kernels' ratio is set from.  A free run is
    chaotic -- the figure moves with torch's summation order -- so the float32 run takes one thread: the same figure on every run."""
    l64, _ = free_run_oracle(oracle, state, batches)
    sub = TorchSubject(oracle, state, oracle.sched, seed_offset=oracle.seed_offset)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        l32 = [sub.train(b, t0, oracle.sched.lr(t0))["loss"] for t0, b in enumerate(batches)]
    finally:
        torch.set_num_threads(threads)
    return float(block_means(l32)[-1] / block_means(l64)[-1])
