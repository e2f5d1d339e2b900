"""Event layouts for tests/test_event_scoring.py: dense events, events pinned to the sweep's pass boundaries, events that outrun their
signal, and the lengths around mining's 64-step probe.  A layout is one signal's sorted, disjoint list of (first, last, label) in steps
(inclusive), as `detection_sweep` and `mine_detections` take it."""
from tests.test_sweep import PASS

STAGED = 256                    # events sweep_kernel stages per round of a pass
PROBE_LENGTHS = (1, 2, 63, 64, 65, 129, 300)        # around mine_event_kernel's 64 steps a probe


def alternating_labels(num_classes):
    """(a, b): the labels of a signal whose top is a on even steps and b on odd ones.  The boundary events below carry them, so that on
    such a signal they are hit at known steps."""
    assert num_classes >= 2
    return num_classes // 2, 0


def boundary_events(steps, num_classes):
    """The four events that follow the one-step events of the n255 .. n513 layouts: one that ends on the last step of pass 0, one that is
    the first step of pass 1 (and touches both neighbours), one that spans three passes, one that runs past the signal's end."""
    a, b = alternating_labels(num_classes)
    return [(PASS - 3, PASS - 1, b), (PASS, PASS, a), (PASS + 1, 3 * PASS + 5, a), (3 * PASS + 10, steps + 50, num_classes - 1)]


def three_pass_event(steps, num_classes):
    return boundary_events(steps, num_classes)[2]


def check_layout(events):
    """Sorted and disjoint, first <= last, from step 0 on: the precondition of every call that takes the layout."""
    for j, (f, l, _) in enumerate(events):
        assert 0 <= f <= l, (j, f, l)
        assert j == 0 or f > events[j - 1][1], (j, events[j - 1], events[j])


def event_layouts(steps, num_classes, rng):
    """name -> layout for a signal of `steps` steps (a signal without steps has no events).  The layouts with pass-boundary events
    need a signal of more than three passes and are left out of shorter ones."""
    C = num_classes
    if steps <= 0:
        return {name: [] for name in ("every_step", "every_other", "adjacent_pairs", "adjacent_triples", "whole_signal", "probe_lengths")}
    a, _ = alternating_labels(C)
    out = {
        "every_step": [(i, i, i % C) for i in range(steps)],
        "every_other": [(i, i, (i // 2) % C) for i in range(0, steps, 2)],
        "adjacent_pairs": [(i, i + 1, (i // 2) % C) for i in range(0, steps - 1, 2)],
        # three steps: the shortest event that can hold a duplicate (two detections in a row never share a label)
        "adjacent_triples": [(i, i + 2, (i // 3) % C) for i in range(0, steps - 2, 3)],
        "whole_signal": [(0, steps + 10, a)],
    }
    if steps > 3 * PASS + 10:
        for k in (255, 256, 257, 512, 513):
            out[f"n{k}"] = [(i, i, i % C) for i in range(k)] + boundary_events(steps, C)
        out["three_pass"] = [three_pass_event(steps, C)]
    probe, pos, j = [], 0, 0
    while pos < steps:                                  # (the last one may outrun the signal)
        m = PROBE_LENGTHS[j % len(PROBE_LENGTHS)]
        probe.append((pos, pos + m - 1, int(rng.randint(C))))
        pos += m + j % 3                                # gaps of 0, 1 and 2 steps
        j += 1
    out["probe_lengths"] = probe
    for ev in out.values():
        check_layout(ev)
    return out
