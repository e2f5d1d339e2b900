"""Front-end framings for tests/test_stream_framings.py: the (window, hop, clip length) geometry the streaming state and the scan
pipeline derive their tail, staging rows and state layout from (stream.hip: StreamGeom; scan.hip: ScanGeom), one row per case.

With  n = clip samples,  T = 1 + (n - win) // hop  frames,  remainder = (n - win) % hop,  a step's new samples start
tail = win - hop + remainder  samples behind its first new frame's first sample.  tail > 0: that many old samples are kept per stream;
tail == 0: none; tail < 0 (hop > win only): the step's first -tail samples lie between two frames and belong to none.  A row states
its (T, remainder, tail) and the test asserts them, so that an edited row cannot drift into another case."""
from collections import namedtuple

Framing = namedtuple("Framing", "name sample_rate clip_ms win hop lower_hz upper_hz num_mfccs method k T remainder tail")

MFCC, LOG_MEL = "mfcc", "log_mel_spectrogram"

ROWS = [
    # ---- tail == 0 and tail > 0
    Framing("hop_eq_win",            16000, 500, 320, 320, 80.0, 7600.0, 40, MFCC, 3, 25, 0, 0),
    Framing("hop_mod4_2",            16000, 500, 640, 322, 80.0, 7600.0, 40, MFCC, 3, 23, 276, 594),       # staging-row stride rounding, 8-byte frame starts
    Framing("hop_gt_win_pos_tail",   16000, 600, 960, 1000, 80.0, 7600.0, 40, MFCC, 2, 9, 640, 600),
    # k hop = 128 < tail: old tail samples survive a call (the scan's tail update keeps them); the tail near its bound of 1024
    Framing("short_call_1024_128",   16000, 205, 1024, 128, 80.0, 7600.0, 40, MFCC, 1, 18, 80, 976),
    Framing("rem_480_250",           16000, 400, 480, 250, 80.0, 7600.0, 40, MFCC, 3, 24, 170, 400),
    Framing("w1024_h1024_32k",       32000, 400, 1024, 1024, 80.0, 7600.0, 40, MFCC, 1, 12, 512, 512),
    # ---- tail < 0: a step starts in the gap between two frames
    Framing("hop_gt_win_neg_tail",   16000, 400, 320, 600, 80.0, 7600.0, 40, MFCC, 2, 11, 80, -200),
    Framing("neg_tail_512_1024",     16000, 630, 512, 1024, 80.0, 7600.0, 40, MFCC, 2, 10, 352, -160),
    Framing("neg_tail_480_962",      16000, 600, 480, 962, 80.0, 7600.0, 40, MFCC, 1, 10, 462, -20),        # the smallest: |tail| < 64, one state alignment unit
    Framing("neg_tail_k_eq_T",       16000, 400, 320, 600, 80.0, 7600.0, 40, MFCC, 11, 11, 80, -200),      # every column new, and a skip
    # ---- tail == 0 from hop > win: remainder == hop - win
    Framing("hop_gt_win_zero_tail",  16000, 1000, 320, 1000, 80.0, 7600.0, 40, MFCC, 2, 16, 680, 0),
    # ---- k = T and k = T - 1 (one surviving column) at hop > win
    Framing("k_eq_T_hop_gt_win",     16000, 500, 640, 700, 80.0, 7600.0, 40, MFCC, 11, 11, 360, 300),
    Framing("k_eq_T_minus_1",        16000, 400, 512, 600, 80.0, 7600.0, 40, MFCC, 9, 10, 488, 400),
    # ---- other feature shapes: 64 log-mel coefficients at a non-reference window (k hop == tail), one MFCC
    Framing("log_mel_960_320",       16000, 400, 960, 320, 80.0, 7600.0, 40, LOG_MEL, 2, 18, 0, 640),
    Framing("one_mfcc_512_384",      16000, 250, 512, 384, 80.0, 7600.0, 1, MFCC, 3, 10, 32, 160),
]
ROW = {r.name: r for r in ROWS}
ROW_IDS = [r.name for r in ROWS]

# (name, sample_rate, clip_ms, win, hop, lower_hz, upper_hz, clip samples): an odd clip length -- the offline front-end runs its general
# kernel on it, which the streaming instance does not reproduce bitwise
REFUSED = [("odd_clip_11025", 11025, 1000, 320, 160, 80.0, 5000.0, 11025),
           ("odd_clip_16001", 16000, 1000.0625, 640, 320, 80.0, 7600.0, 16001)]


def geometry(n_samples, win, hop):
    """(T, remainder, tail) of a clip of n_samples."""
    return 1 + (n_samples - win) // hop, (n_samples - win) % hop, win - hop + (n_samples - win) % hop
