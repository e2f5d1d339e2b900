"""The command lines of enrolled keywords: enroll_audio.py writes the templates `KeywordTemplates.enroll` cuts, scan_audio.py --templates
prints `TemplateDetector.detect`'s detections, stream_audio.py --templates prints exactly the same lines, sweep_audio.py --templates the
detector's curve; the flag is refused next to --phrases and in the chunked runs.  Emulator (`-m "not gpu"`) and MI355X (`-m gpu`)."""
import csv
import io

import numpy as np
import pytest

from tests.test_phrases import cli_case, in_process, same
from tests.test_scan import scanning

SETTINGS = dict(frames_per_step=2, average_window_ms=200, min_count=2, detection_threshold=0.9, suppression_ms=0)


def check_cli(lib, tmp_path, capsys, monkeypatch):
    from tcresnet_amd import enroll_audio, scan_audio, stream_audio, sweep_audio
    from tcresnet_amd.audio_input import Recordings
    Sc = scanning()
    path, wavs = cli_case(lib, tmp_path, 61, lengths=(19200, 19200))
    FrozenModel = in_process(monkeypatch, lib)
    tpl = str(tmp_path / "templates.npz")
    capsys.readouterr()
    assert enroll_audio.main(enroll_audio.parse_arguments(["--frozen", path, "--out", tpl, "--frames_per_step", "2", "--average_window_ms", "200",
                                                           f"first={wavs[0]}:300-700", f"second={wavs[1]}:400-900"])) == 0
    assert enroll_audio.main(enroll_audio.parse_arguments(["--frozen", path, "--out", tpl, "--frames_per_step", "2", "--average_window_ms", "200",
                                                           "--append", "--max_frames", "4", f"first={wavs[1]}:100-420"])) == 0
    said = capsys.readouterr().out.splitlines()
    assert said == [f"first,{wavs[0]},10,300,700", f"second,{wavs[1]},13,400,900", f"first,{wavs[1]},4,100,420"]
    # the file holds the rows of the scan the detecting tools run
    sc = FrozenModel.load(path).scanner(**SETTINGS)
    rec = Recordings(wavs, sc)
    scan = sc.scan_ragged(rec.packed())
    sm = scan.smoothed.cpu().numpy()
    kt = Sc.KeywordTemplates.load(tpl)
    assert kt.names == ["first", "second"] and [len(t) for t in kt.keywords["first"]] == [10, 4]
    same(kt.keywords["first"][0], sm[7:17], "300 .. 700 ms of file 0: steps 7 .. 16 of 40 ms")
    same(kt.keywords["second"][0], sm[30 + 9:30 + 22], "400 .. 900 ms of file 1")
    same(kt.keywords["first"][1], sm[30 + 2:30 + 10:2], "100 .. 420 ms of file 1: eight rows, every other")
    # scan_audio.py --templates: the detector's detections, one line each
    flags = ["--frozen", path, "--wav", *wavs, "--frames_per_step", "2", "--average_window_ms", "200", "--min_count", "2", "--detection_threshold",
             "0.9", "--suppression_ms", "0", "--templates", tpl]
    assert scan_audio.main(scan_audio.parse_arguments([*flags, "--ragged", "--summary"])) == 0
    cap = capsys.readouterr()
    td = Sc.TemplateDetector(sc, kt)
    assert td.max_steps == 39 and abs(td.det.threshold - 0.9) < 1e-6 and td.det.suppression_steps == 0
    det = td.detect(scan)
    top, score, new = det.top.cpu().numpy(), det.score.cpu().numpy(), det.is_new.cpu().numpy()
    want = []
    for p in np.flatnonzero(new):
        n, i = int(p // 30), int(p % 30)
        want.append((i, n, f"{wavs[n]},{round(1000.0 * (i + 1) * 640 / 16000, 3):g},{td.labels[top[p]]},{float(score[p]):.6f}"))
    lines = [line for _, _, line in sorted(want)]
    assert cap.out.splitlines() == lines and len(lines) >= 3 and '"detections": %d' % len(lines) in cap.err
    assert float(det.probs[16, 0]) == 1.0 and float(det.probs[30 + 21, 1]) == 1.0        # where they were cut: exactly 1
    assert {line.split(",")[2] for line in lines} >= {"first", "second"}
    # the padded one-call run and the streams print the same lines
    assert scan_audio.main(scan_audio.parse_arguments(flags)) == 0
    assert capsys.readouterr().out.splitlines() == lines
    assert stream_audio.main(stream_audio.parse_arguments(flags)) == 0
    assert capsys.readouterr().out.splitlines() == lines
    tight = [*flags, "--template_max_stretch", "0.5"]       # at most 7 steps: the 10 and 13 frame templates cannot match at their own rate
    assert scan_audio.main(scan_audio.parse_arguments(tight)) == 0
    short = capsys.readouterr().out.splitlines()
    assert stream_audio.main(stream_audio.parse_arguments(tight)) == 0
    assert capsys.readouterr().out.splitlines() == short != lines
    # sweep_audio.py --templates: the detector's curve
    rows = [(wavs[0], 500, 900, "first"), (wavs[1], 700, 1100, "second")]
    ev_csv = tmp_path / "events.csv"
    ev_csv.write_text("file,start_ms,end_ms,label\n" + "".join(f"{f},{s},{e},{c}\n" for f, s, e, c in rows))
    sweep_flags = ["--frozen", path, "--wav", *wavs, "--frames_per_step", "2", "--average_window_ms", "200", "--min_count", "2", "--suppression_ms",
                   "0", "--events", str(ev_csv), "--thresholds", "0.5,0.9,0.99", "--tolerance_ms", "100", "--templates", tpl, "--ragged"]
    assert sweep_audio.main(sweep_audio.parse_arguments(sweep_flags)) == 0
    got = list(csv.reader(io.StringIO(capsys.readouterr().out)))
    events = [[(s, e, c) for f, s, e, c in rows if f == w] for w in wavs]
    cv = td.sweep(scan, [0.5, 0.9, 0.99], events=events, tolerance_ms=100).curve()
    assert got[0] == list(sweep_audio.COLUMNS) and got[1:] == [[str(x) for x in sweep_audio.format_row(cv, t)] for t in range(3)]
    assert int(cv["events"][0]) == 2 and int(cv["hits"][2]) >= 1
    # refusals, before any model is loaded
    for tool, extra, msg in ((scan_audio, ["--phrases", "1 2"], "--templates and --phrases are two detectors"),
                             (stream_audio, ["--phrases", "1 2"], "--templates and --phrases are two detectors"),
                             (scan_audio, ["--chunk_seconds", "1"], "--templates scores whole scans"),
                             (scan_audio, ["--ragged_chunk_seconds", "1"], "--templates scores whole scans"),
                             (sweep_audio, ["--chunk_seconds", "1"], "--templates scores whole scans")):
        base = sweep_flags[:-1] if tool is sweep_audio else flags
        with pytest.raises(SystemExit, match=msg):
            tool.main(tool.parse_arguments([*base, *extra]))
    with pytest.raises(SystemExit, match="is not NAME=FILE.wav"):
        enroll_audio.main(enroll_audio.parse_arguments(["--frozen", path, "--out", tpl, wavs[0]]))
    assert scan_audio.parse_arguments(flags[:-2]).templates is None


def test_template_command_lines(emu_lib, tmp_path, capsys, monkeypatch):
    check_cli(emu_lib, tmp_path, capsys, monkeypatch)


@pytest.mark.gpu
def test_gpu_template_command_lines(hip_lib, tmp_path, capsys, monkeypatch):
    check_cli(hip_lib, tmp_path, capsys, monkeypatch)
