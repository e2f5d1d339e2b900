"""Training beyond step three (tests/train_walk.py has the method and the reasons).

A. Teacher-forced walks at the engine level: 6 to 24 optimisation steps, every step against the float64 oracle started from the
   state the kernels hold -- logits, losses, every gradient, moving statistics, the optimiser update and its slots, the step size
   that was applied, and every fourth step the eval paths (forward_infer, forward_waveform, a waveform_call prepared before the walk).
B. The trainer: the learning rate and the step counters as the command line sets them, from scratch and across a resume.
C. It trains: train_audio on a learnable WAV directory, evaluate_audio from its checkpoint, next to the float64 oracle on the same batches.
D. Controls (CPU, no kernel): perturbed copies of the oracle through the same comparisons against the float32 torch counterpart.

Every kernel case runs on the emulator build (`-m "not gpu"`) and on the gfx950 library (`-m gpu`)."""
import numpy as np
import pytest
import torch

import tcresnet_amd as T
from oracle import numpy_ref as R
from tests import common as Cm
from tests import train_walk as W


@pytest.fixture(autouse=True, scope="module")
def oracle_threads():
    """At most 16 threads for the oracles' torch work, and no more than a worker's share of the cores when the suite runs on several."""
    import os
    before = torch.get_num_threads()
    workers = int(os.environ.get("PYTEST_XDIST_WORKER_COUNT", "1"))
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 1) // workers)))
    yield
    torch.set_num_threads(before)


@pytest.fixture(params=["emu", pytest.param("hip", marks=pytest.mark.gpu)])
def rt(request):
    """The library the model classes run on: the emulator build on CPU, the gfx950 build on the GPU box."""
    from tcresnet_amd import runtime
    from tcresnet_amd.audio_nets import tc_resnet
    lib = request.getfixturevalue("emu_lib" if request.param == "emu" else "hip_lib")
    runtime.set_default(lib, "cpu" if request.param == "emu" else "cuda")
    tc_resnet.reset_engines()
    yield lib
    runtime.set_default(None, None)
    tc_resnet.reset_engines()


# ---- A. teacher-forced walks ------------------------------------------------------------------------------------------------------
def batch_6_4_6(t0):
    """6 -> 4 -> 6 at steps 10 and 12: the training workspace of batch 6 is taken from engine.py::workspace's cache again after batch 4 ran."""
    return 4 if 10 <= t0 < 12 else 6


def held_waveforms(oracle, b):
    wav = R.synth_waveforms(b, seed=999)
    return {"wav": wav, "x": R.mfcc(wav, oracle.cfg), "labels": R.synth_labels(b).astype(np.float64)}


def tc_walk(lib, sched, steps, name="TCResNet8", width=1.0, tag="4020", held_batch=5, title=""):
    oracle = W.TCOracle(sched, name, width, tag)
    held = held_waveforms(oracle, held_batch)
    fe = Cm.make_frontend(lib, oracle.cfg.win, oracle.cfg.hop)
    state = oracle.init_state()
    net = T.TCResNet(name, R.tcresnet_channels(name, float(width)), 40, fe.n_frames, 12, lib=lib, device=Cm.device_of(lib))
    subject = W.KernelSubject(lib, net, state, sched, frontend=fe, waveform_paths=True, held_out=held)
    w = W.walk(subject, oracle, sched, steps, held, title=title or f"{name}-{width} {sched.opt}")
    return w, subject, oracle, held


def test_walk_tcresnet8_momentum(rt):
    """24 momentum steps across two learning-rate boundaries and a 6 -> 4 -> 6 batch change; then the prepared call's pointer case."""
    sched = W.momentum_schedule([8, 16], [0.1, 0.01, 0.001], batch_6_4_6)
    w, subject, oracle, held = tc_walk(rt, sched, 24)
    assert w.rows["step_size_rel"][0] < W.LR_RTOL
    # The prepared call of the walk's start must have refused at every eval point (the walk asserts refused-or-fresh).  A call
    # prepared NOW runs; after the variables are rebound to another arena and loaded with other weights it refuses or is fresh --
    # it never answers from the arena and the folded table it bound.
    net = subject.net
    out = (torch.zeros_like(subject.call_out[0]), torch.zeros_like(subject.call_out[1]))
    call = net.waveform_call(subject.fe, subject.held_wav, out)
    p, s, _ = subject.read()
    ref = oracle.eval(p, s, held)
    got = subject.run_call(call, out)
    assert got != "refused" and np.abs(got[0] - ref[0]).max() < Cm.LOGIT_TOL * W.eval_scale(ref[0])
    p0, _ = oracle.init_state(seed=11)
    net.params = net.params.clone()
    net.load_state_dict(p0, strict=False)        # (the variables alone: the moving statistics, and their version counter, stay)
    ref2 = oracle.eval(p0, s, held)
    assert np.abs(ref2[0] - ref[0]).max() > 100 * Cm.LOGIT_TOL
    got = subject.run_call(call, out)
    tol = W.eval_scale(ref2[0])
    assert got == "refused" or np.abs(got[0] - ref2[0]).max() < Cm.LOGIT_TOL * tol, "a prepared waveform_call answered with the weights of a rebound arena"
    for path, (lg, pr) in {k: v for k, v in subject.evals(held).items() if k != "waveform_call"}.items():
        assert np.abs(lg - ref2[0]).max() < Cm.LOGIT_TOL * tol and np.abs(pr - ref2[1]).max() < W.PROB_TOL, path


def test_walk_tcresnet8_adam(rt):
    """24 Adam steps: t reaches 24, where t and t +- 1 are 1.2 % apart in the applied step size."""
    tc_walk(rt, W.adam_schedule(0.01, lambda t0: 6), 24)


def test_walk_tcresnet8_rmsprop_ema(rt):
    """12 RMSProp steps (decay 0.8, momentum 0.5, epsilon 1e-3) with the EMA shadow stepped behind each."""
    tc_walk(rt, W.rmsprop_schedule(0.001, lambda t0: 6), 12)


def test_walk_tcresnet14_wide_momentum(rt):
    """TCResNet14-1.5 at 98 frames (30 / 10 ms), batch 5, momentum across one boundary: identity shortcuts, the per-layer backward.
    12 steps on the GPU; the emulator needs ~10 s per step at this size and walks 6."""
    steps = 6 if rt.kind == "emu" else 12
    sched = W.momentum_schedule([steps // 2 - 1], [0.1, 0.01], lambda t0: 5)
    tc_walk(rt, sched, steps, name="TCResNet14", width=1.5, tag="3010", held_batch=3)


def test_walk_dscnn_s_adam(rt):
    """DS-CNN-S, 12 Adam steps against oracle/dscnn_ref.py: conv biases ahead of a train-mode BN keep an exactly zero gradient."""
    sched = W.adam_schedule(5e-4, lambda t0: 6)
    sched.keep_prob = 1.0               # (the graph has no dropout)
    oracle = W.DSOracle(sched, "S")
    held = held_waveforms(oracle, 5)
    fe = Cm.make_frontend(rt, oracle.cfg.win, oracle.cfg.hop, num_mfccs=10)
    net = T.DSCNN("S", fe.n_frames, 10, 12, lib=rt, device=Cm.device_of(rt))
    subject = W.KernelSubject(rt, net, oracle.init_state(), sched, frontend=fe)
    # (twelve candidates, as check_dscnn_train_live takes: W.DSOracle has the measurement)
    W.walk(subject, oracle, sched, 12, held, k_cands=12, title="DS-CNN-S adam")


def test_walk_res8narrow_momentum(rt):
    """Res8Narrow on the graph engine (19 channels, 4 x 3 average pool, BN without centre / scale), 8 momentum steps across one boundary
    against oracle/net2d_ref.py."""
    from tcresnet_amd.audio_nets import res
    from tests.test_g2d_configs import GRAD_RTOL as G2D_GRAD_RTOL
    t, f, b = (12, 10, 3) if rt.kind == "emu" else (20, 12, 3)
    eng = res.get_engine("Res8Narrow", t, f, 12)
    eng.init_variables(4)
    sd = {k: v.astype(np.float64) for k, v in eng.state_dict().items() if k in eng.tensors}
    p = {k: v for k, v in sd.items() if eng.tensors[k].arena == 0}
    s = {k: v for k, v in sd.items() if eng.tensors[k].arena == 1}
    sched = W.momentum_schedule([3], [0.1, 0.01], lambda t0: b)
    sched.keep_prob = 1.0               # (no dropout node in this graph)
    decays = [k for k in p if eng.tensors[k].offset < eng.n_decay]
    oracle = W.G2DOracle(sched, "Res8Narrow", t, f, decays, G2D_GRAD_RTOL)
    held = oracle.make_batch(4, 1000, 0)
    subject = W.KernelSubject(rt, eng, (p, s), sched)
    W.walk(subject, oracle, sched, 8, held, title="Res8Narrow momentum")


# ---- D. controls on the oracle side (no kernel) -------------------------------------------------------------------------------------
# Each perturbed copy of the oracle restates ONE expectation wrongly -- the defect a kernel-side bug of that kind would amount to --
# and goes through walk()'s comparisons against the float32 torch counterpart of the clean oracle.  The comparison that is there to
# catch it must be exceeded at least tenfold; the clean oracle stays under every bound.
class ShiftedBoundary(W.TCOracle):
    def lr(self, t0):
        return self.sched.lr(t0 - 1)


class AdamOffByOne(W.TCOracle):
    def opt_t(self, t0):
        return t0 + 1 if t0 + 1 < 10 else t0 + 2          # from the tenth step on


class StuckDropoutSeed(W.TCOracle):
    def seed(self, t0):
        return 0


class FrozenStatistics(W.TCOracle):
    def new_stats(self, s, rec, t0):
        return rec["new_stats"] if t0 == 0 else s


class ZeroedMomentum(W.TCOracle):
    def update(self, p, g, slots, t0):
        return super().update(p, g, {n: {k: np.zeros_like(v) for k, v in d.items()} for n, d in slots.items()}, t0)


class StaleEval(W.TCOracle):
    def forward(self, p, s, batch, t0):
        self.before_step = (p, s)
        return super().forward(p, s, batch, t0)

    def eval_state(self, p, s):
        return self.before_step


CONTROL_SCHEDULES = {"mom": (lambda: W.momentum_schedule([3, 6], [0.1, 0.01, 0.001], lambda t0: 6), 10),
                     "adam": (lambda: W.adam_schedule(0.01, lambda t0: 6), 12)}
CONTROLS = [("clean_momentum", W.TCOracle, "mom", None), ("clean_adam", W.TCOracle, "adam", None),
            ("boundary_shifted_by_one", ShiftedBoundary, "mom", "step_size_rel"), ("adam_t_off_by_one_from_step_10", AdamOffByOne, "adam", "opt_params"),
            ("dropout_seed_not_advancing", StuckDropoutSeed, "mom", "train_logits"), ("moving_statistics_frozen", FrozenStatistics, "mom", "moving_stats"),
            ("momentum_slot_zeroed", ZeroedMomentum, "mom", "step_params"), ("eval_from_previous_weights", StaleEval, "mom", "eval_logits")]


@pytest.mark.parametrize("name,cls,opt,caught_by", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_control(name, cls, opt, caught_by):
    make, steps = CONTROL_SCHEDULES[opt]
    sched = make()
    oracle = cls(sched)
    subject = W.TorchSubject(oracle, oracle.init_state(), sched)
    w = W.walk(subject, oracle, sched, steps, held_waveforms(oracle, 5), check=False, title=f"control {name}")
    ratios = {q: w.ratio(q) for q in w.rows}
    print(name, {q: f"{r:.3g}" for q, r in ratios.items()})
    if caught_by is None:
        assert max(ratios.values()) < 1.0, ratios
    else:
        assert ratios[caught_by] >= 10.0, (name, caught_by, ratios[caught_by])


# ---- B. the trainer: schedule and counters as the command line sets them ----------------------------------------------------------
def make_trainer(cmd, train_dir, num_samples=None):
    """SingleLabelAudioTrainer on TCResNet8Model over the synthetic dataset, built as train_audio.train builds it."""
    from tcresnet_amd import train_audio
    from tcresnet_amd.audio_nets import tc_resnet
    from tcresnet_amd.datasets.synthetic import SyntheticAudioDataWrapper
    from tcresnet_amd.factory import audio_nets
    from tcresnet_amd.helper.trainer import SingleLabelAudioTrainer
    tc_resnet.reset_engines()
    args = train_audio.parse_arguments(cmd.format(d=train_dir).split())
    ds = SyntheticAudioDataWrapper(args, None, "train", True, **({} if num_samples is None else {"num_samples": num_samples}))
    wavs, labels = ds.get_input_and_output_op()
    model = audio_nets.TCResNet8Model(args, ds)
    model.build(wavs, labels, is_training=True)
    return SingleLabelAudioTrainer(model, None, args, ds, "train")


def stepped(tr, opt, steps, boundaries, lr_list, save_at=None):
    """run_single_step `steps` times; before and after each, the variables and slots are read; the step size recovered from them must
    be the schedule's at global_step BEFORE the step (Adam: times the bias correction at t = global_step + 1), and the model's step
    counter -- Adam's t, the dropout seed -- must equal global_step."""
    eng = tr.model.engine
    hp = {"mu": 0.9, "b1": 0.9, "b2": 0.999, "eps": 1e-8}
    arenas = lambda: ({"all": eng.params.cpu().numpy().astype(np.float64)}, {n: {"all": eng.slot_arena(n).cpu().numpy().astype(np.float64)} for n in W.SLOTS[opt]})
    seen = []
    for _ in range(steps):
        g0 = tr.global_step
        assert tr.model.step_count() == g0
        p0, s0 = arenas()
        _, _, lr_used, _ = tr.run_single_step()
        p1, s1 = arenas()
        step, _ = W.applied_step(opt, hp, ["all"], p0, p1, None, s0, s1)
        want = R.piecewise_constant_lr(g0, boundaries, lr_list) * (W.adam_factor(hp, g0 + 1) if opt == "adam" else 1.0)
        seen.append((g0, step, want))
        assert abs(step / want - 1.0) < W.LR_RTOL, f"global_step {g0}: applied step size {step:.6g}, the schedule says {want:.6g} ({seen})"
        assert tr.global_step == g0 + 1 == tr.model.step_count()
        if save_at == tr.global_step:
            tr.save()
    return seen


def trainer_cmd(boundaries="--boundaries 3 6", schedule="--absolute_schedule", extra=""):
    from tests.test_boundary import REF_TRAIN_CMD
    return REF_TRAIN_CMD.replace("--boundaries 2 4", boundaries).replace("--absolute_schedule", f"{schedule} {extra}")


def test_trainer_schedule_from_scratch_and_resumed(rt, tmp_path):
    """--boundaries 3 6 --lr_list 0.1 0.01 0.001: nine steps from scratch; then resumed from the checkpoint of step 4 -- with
    --relative_schedule the boundaries move to 7 and 10, with --absolute_schedule they stay."""
    lrs = [0.1, 0.01, 0.001]
    tr = make_trainer(trainer_cmd(), tmp_path / "a")
    seen = stepped(tr, "mom", 9, [3, 6], lrs, save_at=4)
    assert [round(w, 6) for _, _, w in seen] == [0.1] * 4 + [0.01] * 3 + [0.001] * 2
    for schedule, bounds, want in (("--relative_schedule", [7, 10], [0.1] * 4 + [0.01] * 3), ("--absolute_schedule", [3, 6], [0.01] * 3 + [0.001] * 4)):
        tr = make_trainer(trainer_cmd(schedule=schedule, extra=f"--checkpoint_path {tmp_path / 'a'}"), tmp_path / schedule.strip("-"))
        assert tr.global_step == 4 == tr.global_step_from_checkpoint and tr.boundaries == bounds
        seen = stepped(tr, "mom", 7, bounds, lrs)
        assert [g for g, _, _ in seen] == list(range(4, 11)) and [round(w, 6) for _, _, w in seen] == want


def test_trainer_epoch_boundaries(rt, tmp_path):
    """--boundaries_epoch: boundary b (in epochs) falls at step b * num_samples // batch_size.  The synthetic split is given 10 samples so
    that, at the batch of 3 these tests use, the boundaries 1 and 2 fall at steps 3 and 6."""
    tr = make_trainer(trainer_cmd("--boundaries 1 2").replace("--no-boundaries_epoch", "--boundaries_epoch"), tmp_path / "e", num_samples=10)
    bounds = [b * tr.dataset.num_samples // tr.dataset.batch_size for b in (1, 2)]
    assert bounds == [3, 6] and tr.boundaries == bounds
    stepped(tr, "mom", 8, bounds, [0.1, 0.01, 0.001])


def test_trainer_adam_ema_counters_across_resume(rt, tmp_path):
    """--optimizer adam --use_ema: Adam's t and the dropout seed (model.step_count()) continue from the restored global_step."""
    lrs = [0.01, 0.005, 0.001]
    cmd = trainer_cmd().replace("--optimizer mom --momentum 0.9", "--optimizer adam --use_ema --ema_decay 0.9").replace("--lr_list 0.1 0.01 0.001", "--lr_list 0.01 0.005 0.001")
    tr = make_trainer(cmd, tmp_path / "a")
    stepped(tr, "adam", 5, [3, 6], lrs, save_at=5)
    ema = tr.model.engine.slots["ExponentialMovingAverage"].clone()
    tr = make_trainer(cmd.replace("--optimizer adam", f"--checkpoint_path {tmp_path / 'a'} --optimizer adam"), tmp_path / "b")
    assert tr.global_step == 5 and tr.model.step_count() == 5
    assert torch.equal(tr.model.engine.slots["ExponentialMovingAverage"], ema)
    seen = stepped(tr, "adam", 7, [3, 6], lrs)
    assert [g for g, _, _ in seen] == list(range(5, 12))


# ---- C. it trains: WAV files -> train_audio -> checkpoint -> evaluate_audio ----------------------------------------------------------
TRAIN_CMD = ("--dataset_path {data} --dataset_split_name train --output_name output/softmax --num_classes 12 --train_dir {d} --num_silent {per} --no-shuffle "
             "--augmentation_method anchored_slice_or_pad --preprocess_method mfcc --num_mfccs 40 --clip_duration_ms 1000 --window_size_ms 40 "
             "--window_stride_ms 20 --background_frequency 0.0 --background_max_volume 0.0 --batch_size {batch} --boundaries {half} "
             "--max_step_from_restore {steps} --lr_list 0.1 0.01 --absolute_schedule --no-boundaries_epoch --max_to_keep 2 "
             "--step_save_checkpoint 100000 --step_evaluation 100000 --optimizer mom --momentum 0.9 --step_save_summaries 100000 "
             "TCResNet8Model --weight_decay 0.001 --width_multiplier 1.0")
EVAL_CMD = ("--dataset_path {data} --dataset_split_name valid --output_name output/softmax --num_classes 12 --checkpoint_path {d} --num_silent 2 "
            "--augmentation_method anchored_slice_or_pad --preprocess_method mfcc --num_mfccs 40 --clip_duration_ms 1000 --window_size_ms 40 "
            "--window_stride_ms 20 --background_frequency 0.0 --background_max_volume 0.0 --max_step_from_restore 30000 --batch_size 12 "
            "--no-shuffle --valid_type once --evaluation_iterations 2 TCResNet8Model --weight_decay 0.001 --width_multiplier 1.0")
# Mean model loss of the last sixth of the run, float32 torch oracle over float64 oracle on these recipes with dropout on (the same
# batches and masks, on the CPU; the kernels do not enter).  A free run is chaotic, so the figure moves with torch's summation order:
# batch 12 x 30 steps 1.18 at 1, 8 and 16 threads; batch 24 x 60 steps 1.58 at 1 thread, 1.01 at 8, 1.30 at 16.  Recorded: the one-thread
# figures, which W.float32_loss_ratio reproduces run after run (test_loss_ratio_bound_comes_from_the_float32_oracle) and which are the
# largest seen.  m = 1.5 x the largest, not below 2.
LOSS_RATIO_MEASURED = {"emu": 1.18, "hip": 1.58}
LOSS_RATIO_BOUND = max(2.0, 1.5 * max(LOSS_RATIO_MEASURED.values()))


def it_trains_recipe(kind):
    """(batch, steps, clips per word): 24 x 60 on the GPU, 12 x 30 on the emulator (about 2 s per step there).  The train split holds
    exactly one batch -- clips per word x 11 words + as many silent samples: --no-shuffle orders a split label by label, so only a batch
    that spans the split sees every class."""
    return (12, 30, 1) if kind == "emu" else (24, 60, 2)


def it_trains_setup(lib, tmp_path, kind):
    """(train_audio arguments, oracle, initial state, steps) of a recipe: the WAV directory written, the oracle on the trainer's schedule
    and dropout seeds, and the initialisation the model classes start from (audio_nets/tc_resnet.py::get_engine)."""
    from tcresnet_amd import train_audio
    batch, steps, per = it_trains_recipe(kind)
    W.write_tone_dataset(tmp_path / "data", {"train": per, "valid": 2})
    args = train_audio.parse_arguments(TRAIN_CMD.format(data=tmp_path / "data", d=tmp_path / "ckpt", batch=batch, steps=steps, half=steps // 2, per=per).split())
    oracle = W.TCOracle(W.momentum_schedule([steps // 2], [0.1, 0.01], lambda t0: batch))
    oracle.seed_offset = 1              # the trainer seeds its dropout with the 1-based step count
    fresh = T.TCResNet("TCResNet8", R.tcresnet_channels("TCResNet8", 1.0), 40, 49, 12, lib=lib, device=Cm.device_of(lib))
    fresh.init_xavier(0)
    sd, (tp, ts) = fresh.state_dict(), oracle.init_state()
    state = ({k: sd[k].astype(np.float64).reshape(v.shape) for k, v in tp.items()}, {k: sd[k].astype(np.float64) for k in ts})
    return args, oracle, state, steps


@pytest.mark.parametrize("kind", ["emu", "hip"])
def test_loss_ratio_bound_comes_from_the_float32_oracle(emu_lib, tmp_path, kind):
    """Where LOSS_RATIO_MEASURED comes from (CPU only; the emulator serves the dataset's input stage, no network kernel runs): the float32
    torch oracle's last-sixth loss over the float64 oracle's on each recipe's own batches.  Asserted: a faithful float32 implementation is
    itself inside the bound set for the kernels (the figure, printed, is chaotic across machines; here 1.18 and 1.58)."""
    from tcresnet_amd import runtime
    from tcresnet_amd.datasets.audio_data_wrapper import SingleLabelAudioDataWrapper
    runtime.set_default(emu_lib, "cpu")
    try:
        args, oracle, state, steps = it_trains_setup(emu_lib, tmp_path, kind)
        ds = SingleLabelAudioDataWrapper(args, None, "train", True)
        ratio = W.float32_loss_ratio(oracle, state, [oracle.batch_of(w, l) for w, l in W.dataset_batches(ds, steps)])
    finally:
        runtime.set_default(None, None)
    print("float32 / float64 last-sixth loss ratio,", kind, "recipe:", ratio)
    assert ratio <= LOSS_RATIO_BOUND, (kind, ratio, LOSS_RATIO_MEASURED[kind])


def test_it_trains_from_wav_files_next_to_the_oracle(rt, tmp_path, monkeypatch):
    """train_audio on a learnable 12-class WAV directory (11 tone classes + silence), momentum 0.9, wd 1e-3, lr 0.1 -> 0.01 at half the
    steps, one checkpoint at the end; evaluate_audio from that checkpoint on the valid split (other clips).  The float64 oracle trains
    on the same batches -- read from the trainer's own dataset object -- with the same dropout masks and the same initialisation.
    (a) block means of the model loss over sixths of the run fall from block to block, for the oracle and then for the kernels;
    (b) the kernels' mean loss over the last sixth is at most LOSS_RATIO_BOUND times the oracle's; (c) valid accuracy is at least the
    oracle's minus one utterance -- which, this early (BN decay 0.997: the moving statistics are 9 to 17 % of the way), shows that
    the two agree, not that either classifies."""
    from tcresnet_amd import evaluate_audio, train_audio
    from tcresnet_amd.datasets.audio_data_wrapper import SingleLabelAudioDataWrapper
    from tcresnet_amd.helper.trainer import SingleLabelAudioTrainer
    args, oracle, state, steps = it_trains_setup(rt, tmp_path, rt.kind)
    kernel_losses = []
    run = SingleLabelAudioTrainer.run_single_step

    def recording(self):
        out = run(self)
        kernel_losses.append(float(out[1]))
        return out
    monkeypatch.setattr(SingleLabelAudioTrainer, "run_single_step", recording)
    trainer = train_audio.train(args)
    assert trainer.global_step == steps == len(kernel_losses)
    assert sorted(p.name for p in (tmp_path / "ckpt").iterdir()) == [f"TCResNet8Model-{steps}.data-00000-of-00001", f"TCResNet8Model-{steps}.index", "checkpoint"]
    out = evaluate_audio.main(evaluate_audio.parse_arguments(EVAL_CMD.format(data=tmp_path / "data", d=tmp_path / "ckpt").split()))
    assert out["step"] == steps and out["num_evaluated"] == 24
    # the oracle on the same batches
    batches = [oracle.batch_of(w, l) for w, l in W.dataset_batches(trainer.dataset, steps)]
    oracle_losses, (p, s) = W.free_run_oracle(oracle, state, batches)
    vargs = evaluate_audio.parse_arguments(EVAL_CMD.format(data=tmp_path / "data", d=tmp_path / "ckpt").split())
    valid = SingleLabelAudioDataWrapper(vargs, None, "valid", False)
    ref_hits = 0
    for w, l in W.dataset_batches(valid, 2):
        ref_hits += int((oracle.eval(p, s, oracle.batch_of(w, l))[0].argmax(1) == l.argmax(1)).sum())
    ob, kb = W.block_means(oracle_losses), W.block_means(kernel_losses)
    print("it trains:", rt.kind, "oracle block means", ob, "kernel block means", kb, "last-sixth ratio", kb[-1] / ob[-1],
          "valid accuracy oracle", ref_hits / 24, "kernels", out["accuracy"])
    assert np.all(np.diff(ob) < 0), ("the oracle's own loss does not fall block to block", ob)
    assert np.all(np.diff(kb) < 0), ("the kernels' loss does not fall block to block", kb, ob)
    assert kb[-1] <= LOSS_RATIO_BOUND * ob[-1], (kb[-1], ob[-1])
    assert out["accuracy"] >= (ref_hits - 1) / 24 - 1e-9, (out["accuracy"], ref_hits / 24)
