"""The pending-reset rule every streaming class shares (tcresnet_amd.detection.PendingResets, reset_mask), on a stub of three streams:
host only, no library and no GPU."""
import numpy as np
import pytest
import torch

import tcresnet_amd as T
from tcresnet_amd.detection import PendingResets, reset_mask

S = 3


class Stub(PendingResets):
    def __init__(self):
        self.n_streams = S
        self._init_resets(torch.device("cpu"))


def flags(stub):
    return None if stub._pending is None else stub._pending.tolist()


def test_mask_and_index_forms():
    for arg in (np.array([False, True, False]), np.array([0, 1, 0], np.uint8), torch.tensor([False, True, False]), [1], (1,), {1},
                np.array([1], np.int64), torch.tensor([1, 1], dtype=torch.int32)):
        m = reset_mask(arg, S)
        assert m.dtype == np.bool_ and m.tolist() == [False, True, False]
    assert reset_mask([], S).tolist() == [False] * S
    assert reset_mask([2, 0], S).tolist() == [True, False, True]
    from tcresnet_amd.streaming import reset_mask as from_streaming
    assert from_streaming is reset_mask


def test_refusals():
    stub = Stub()
    with pytest.raises(T.TcrError, match=r"reset mask must have 3 entries, got shape \(4,\)"):
        stub.reset(np.zeros(4, bool))
    with pytest.raises(T.TcrError, match=r"reset mask must have 3 entries, got shape \(2,\)"):
        stub.reset(np.ones(2, np.uint8))
    for bad in ([3], [-1], [0, 5]):
        with pytest.raises(T.TcrError, match="reset: stream index outside 0..2"):
            stub.reset(bad)
    assert stub._pending is None


def test_accumulates_and_take_clears():
    stub = Stub()
    assert stub._take_reset() is None and stub._begin_ragged_reset() is None
    stub.reset([1])
    assert flags(stub) == [False, True, False]
    stub.reset(np.array([True, False, False]))
    assert flags(stub) == [True, True, False]
    stub.reset([1])
    assert flags(stub) == [True, True, False]
    assert stub._take_reset() == stub._reset_dev.data_ptr()
    assert stub._reset_dev.dtype == torch.uint8 and stub._reset_dev.tolist() == [1, 1, 0]
    assert stub._pending is None and stub._take_reset() is None
    stub.reset([2])                                             # (the device flags are rewritten whole, not OR-ed into)
    stub._take_reset()
    assert stub._reset_dev.tolist() == [0, 0, 1]


def test_ragged_pair_keeps_the_streams_without_rows():
    stub = Stub()
    stub.reset([0, 1])
    assert stub._begin_ragged_reset() == stub._reset_dev.data_ptr()
    assert stub._reset_dev.tolist() == [1, 1, 0] and flags(stub) == [True, True, False]        # (pending until the call has run)
    stub._end_ragged_reset(np.array([4, 0, 0]))
    assert flags(stub) == [False, True, False]                  # stream 0 had rows; stream 2 had none, and no flag either
    stub.reset([2])
    assert stub._begin_ragged_reset() is not None and stub._reset_dev.tolist() == [0, 1, 1]
    stub._end_ragged_reset([0, 2, 0])
    assert flags(stub) == [False, False, True]
    stub._begin_ragged_reset()
    stub._end_ragged_reset([1, 0, 7])
    assert stub._pending is None
    stub._end_ragged_reset([0, 0, 0])                           # (nothing pending: nothing to keep)
    assert stub._pending is None
