"""The three network classes' initial variables and public surface, pinned against literals (emulator build only).

DIGESTS and SURFACE below were produced by running this same test body on the revision BEFORE the three families of `engine.py` got their
common base class, and pasting what it printed; they are never regenerated from the code under test.  A refactor of the engine leaves them
as they are: the initialisers draw from one `torch.Generator` in tensor-table order with particular shapes and dtypes, and every public
method keeps its name, parameters and defaults (`parallel.py` passes one set of keywords to all three families).  `model_ref` is the one
method the base class added; its signature is the one the detection layer calls.
"""
import hashlib
import inspect

import numpy as np

import tcresnet_amd as T

DIGESTS = {
    "TCResNet/constructed": "e855784f079ee81e7c806301b4a742cd31f3edc6928d9408d05a52041432d17d",
    "TCResNet/seed3": "bd68251bb467798e19823ee0d70d46d5f4a745e91d858aabddfd4c6f3ef63dd2",
    "DSCNN/constructed": "3902163eda7badfed62d3330e69ab26c2738e881eca94890d6f99e8cc7e8ff09",
    "DSCNN/seed3": "a2aa3e690f1b9bd4802859ba3f80ce3c9953b2588fb27d66dd6820a50143f8d5",
    "Graph2D/constructed": "227c6cc440fad1b96c7383209d4bb11be5a6927f854085adbf0a99612e28c63e",
    "Graph2D/seed3": "b4ed86fc2a69a94b4eb8150229c4a72853faebfa07d2d916d0a9afdea1f07b8c",
}

ADDED = {"model_ref": "(self, aux: 'Optional[torch.Tensor]' = None) -> '_lib.ModelRef'"}

SHARED = {          # printed identically for all three classes
    "adam_step": "(self, lr: 'float', step: 'int', beta1: 'float' = 0.9, beta2: 'float' = 0.999, eps: 'float' = 1e-08, "
                 "weight_decay: 'float' = 0.0, grad_scale: 'float' = 1.0)",
    "backward": "(self) -> 'torch.Tensor'",
    "ema_init": "(self)",
    "ema_step": "(self, decay: 'float')",
    "grad_view": "(self, name: 'str') -> 'torch.Tensor'",
    "l2_loss": "(self, weight_decay: 'float') -> 'torch.Tensor'",
    "load_state_dict": "(self, sd: 'Dict[str, np.ndarray]', strict: 'bool' = True)",
    "rmsprop_step": "(self, lr: 'float', decay: 'float' = 0.9, momentum: 'float' = 0.0, eps: 'float' = 1e-10, weight_decay: 'float' = 0.0, "
                    "grad_scale: 'float' = 1.0)",
    "sgd_momentum_step": "(self, lr: 'float', momentum: 'float' = 0.9, weight_decay: 'float' = 0.0, grad_scale: 'float' = 1.0)",
    "slot_arena": "(self, name: 'str') -> 'torch.Tensor'",
    "state_dict": "(self) -> 'Dict[str, np.ndarray]'",
    "tf_shape": "(self, name: 'str') -> 'Tuple[int, ...]'",
    "total_params": "(self) -> 'int'",
    "trainable_names": "(self) -> 'List[str]'",
}

FORWARD_TRAIN = ("(self, feat: 'torch.Tensor', labels: 'torch.Tensor', keep_prob: 'float' = 1.0, seed: 'int' = 0, sample_offset: 'int' = 0, "
                 "global_batch: 'Optional[int]' = None, label_smoothing: 'float' = 0.0, sync_hook=None)")

SURFACE = {
    "TCResNet": dict(SHARED, **{
        "fold_bn": "(self) -> 'torch.Tensor'",
        "forward_frozen": "(self, feat: 'torch.Tensor', frozen_ss: 'torch.Tensor', want_ranges: 'bool' = False)",
        "forward_infer": "(self, feat: 'torch.Tensor', want_ranges: 'bool' = False, out=None, workspace: 'Optional[torch.Tensor]' = None)",
        "forward_train": FORWARD_TRAIN,
        "forward_waveform": "(self, frontend: \"'Frontend'\", wav: 'torch.Tensor', want_ranges: 'bool' = False, out=None, "
                            "feat: 'Optional[torch.Tensor]' = None)",
        "init_xavier": "(self, seed: 'int' = 0)",
        "invalidate_folded": "(self)",
        "new_workspace": "(self, batch: 'int', train: 'bool') -> 'torch.Tensor'",
        "reset_bn": "(self)",
        "waveform_call": "(self, frontend: \"'Frontend'\", wav: 'torch.Tensor', out, feat: 'Optional[torch.Tensor]' = None)",
        "workspace": "(self, batch: 'int', train: 'bool') -> 'torch.Tensor'",
    }),
    "DSCNN": dict(SHARED, **{
        "forward_infer": "(self, feat: 'torch.Tensor')",
        "forward_train": "(self, feat: 'torch.Tensor', labels: 'torch.Tensor', global_batch: 'Optional[int]' = None, "
                         "label_smoothing: 'float' = 0.0, **_unused)",
        "from_def": "(depth: 'int', n_separable: 'int', conv1_stride, ds1_stride, h_in: 'int', w_in: 'int', num_classes: 'int', "
                    "conv1_kh: 'int' = 10, **kw)",
        "init_xavier": "(self, seed: 'int' = 0)",
        "train_workspace": "(self, batch: 'int') -> 'torch.Tensor'",
        "unit_output": "(self, unit: 'int', batch: 'int') -> 'torch.Tensor'",
    }),
    "Graph2D": dict(SHARED, **{
        "add": "(self, a: 'int', b: 'int', relu: 'bool' = False) -> 'int'",
        "batch_norm": "(self, inp: 'int', prefix: 'str', center: 'bool' = True, scale: 'bool' = True, relu: 'bool' = False, "
                      "decay: 'float' = 0.997, eps: 'float' = 0.001) -> 'int'",
        "conv": "(self, inp: 'int', kernel, cout: 'int', weights_name: 'str', stride=(1, 1), rate=(1, 1), padding: 'str' = 'SAME', "
                "relu: 'bool' = False, biases_name: 'Optional[str]' = None, init='xavier', tf_shape: 'Optional[Sequence[int]]' = None) -> 'int'",
        "dropout": "(self, inp: 'int', keep_prob: 'float') -> 'int'",
        "finalize": "(self, logits: 'int')",
        "forward_infer": "(self, feat: 'torch.Tensor')",
        "forward_train": FORWARD_TRAIN,
        "group_sum": "(self, inp: 'int', group: 'int', relu: 'bool' = False, biases_name: 'Optional[str]' = None) -> 'int'",
        "init_variables": "(self, seed: 'int' = 0)",
        "input_from_features": "(self, feat: 'torch.Tensor') -> 'torch.Tensor'",
        "node_output": "(self, node: 'int', batch: 'int', train: 'bool') -> 'torch.Tensor'",
        "pool": "(self, inp: 'int', kind: 'str', kernel=None, stride=(1, 1), padding: 'str' = 'VALID') -> 'int'",
        "shape": "(self, node: 'int') -> 'Tuple[int, int, int]'",
        "time_filter": "(self, inp: 'int', weights_name: 'str', init='xavier') -> 'int'",
        "workspace": "(self, batch: 'int', train: 'bool') -> 'torch.Tensor'",
    }),
}


def smallest_nets(lib):
    tc = T.TCResNet("TCResNet", [4, 6], 5, 16, 3, lib=lib, device="cpu")
    ds = T.DSCNN.from_def(8, 1, (2, 2), (1, 1), 16, 8, 3, lib=lib, device="cpu")
    g = T.Graph2D("", 6, 5, 1, lib=lib, device="cpu")
    a = g.batch_norm(g.conv(-1, (3, 3), 4, "conv/weights"), "conv/BatchNorm", relu=True)
    g.finalize(g.conv(g.pool(a, "avg"), (1, 1), 3, "fc/weights", biases_name="fc/biases"))
    return tc, ds, g


def digest(net):
    """sha256 over the float32 bytes of the variable arena followed by the statistics arena."""
    h = hashlib.sha256()
    for arena in (net.params, net.stats):
        h.update(np.ascontiguousarray(arena.detach().cpu().numpy(), np.float32).tobytes())
    return h.hexdigest()


def surface(cls):
    """Public callable name -> its signature as text (annotations and defaults included)."""
    return {n: str(inspect.signature(getattr(cls, n))) for n in sorted(dir(cls)) if not n.startswith("_") and callable(getattr(cls, n))}


def test_initial_variables_and_public_surface(emu_lib):
    tc, ds, g = smallest_nets(emu_lib)
    got = {}
    for net in (tc, ds, g):
        name = type(net).__name__
        got[name + "/constructed"] = digest(net)
        (net.init_variables if name == "Graph2D" else net.init_xavier)(3)
        got[name + "/seed3"] = digest(net)
    print("DIGESTS =", repr(got))
    faces = {cls.__name__: surface(cls) for cls in (T.TCResNet, T.DSCNN, T.Graph2D)}
    print("SURFACE =", repr(faces))
    assert got == DIGESTS
    for name, face in faces.items():
        want = dict(SURFACE[name], **ADDED)
        assert face == want, (name, {k: (face.get(k), want.get(k)) for k in set(face) | set(want) if face.get(k) != want.get(k)})
