"""bench.py's two kinds of run: a plain run does only what the headline line needs (set up, warm up, time the steps, write
--dump-outputs, print); --full also measures and checks everything beside it (bench.FULL_ONLY).  CPU: how the options resolve;
GPU: a small plain run in a fresh process prints the line without the extras, and an option given explicitly still runs its part."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SMALL = ["--volume", "64", "--width", "640", "--height", "368", "--steps", "20", "--warmup", "4"]


def test_a_plain_run_turns_every_extra_off():
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False
    assert {n: getattr(a, n) for n in bench.FULL_ONLY} == {n: 0 for n in bench.FULL_ONLY}


def test_full_turns_every_extra_on():
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert {n: getattr(a, n) for n in bench.FULL_ONLY} == {"check": 1, "stream_probe": 1, "kernels_alone": 1, "other_configs": 1,
                                                          "cpu_baseline": 1, "bucket_form": 1, "display_form": 1, "cadence_form": 16}


def test_an_explicit_value_wins_over_either_default():
    a = bench.parse(["--full", "--other-configs", "0", "--cadence-form", "8"])
    assert a.other_configs == 0 and a.cadence_form == 8 and a.check == 1 and a.cpu_baseline == 1
    b = bench.parse(["--check", "1"])
    assert b.check == 1 and b.cpu_baseline == 0 and b.other_configs == 0


def test_the_timed_steps_do_not_depend_on_full():
    """what the timed region reads is the same in both kinds of run"""
    plain, full = vars(bench.parse(["--steps", "20", "--warmup", "5"])), vars(bench.parse(["--steps", "20", "--warmup", "5", "--full"]))
    differ = {k for k in plain if plain[k] != full[k]}
    assert differ == {"full"} | set(bench.FULL_ONLY)


def _run_bench(extra, timeout=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone(tmp_path):
    line = _run_bench(["--dump-outputs", str(tmp_path)])
    assert all(k in line for k in HEADLINE_KEYS)
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True and line["steps"] == 20
    assert line["value"] == pytest.approx(line["config"]["samples_per_step"] / (line["ms_per_step"] * 1e-3))
    assert line["frame_check"] is None                                   # nothing was compared
    assert not {"cpu_baseline", "cpu_baseline_js", "host_cores", "other_configs"} & set(line)
    assert "per_kernel" not in line["roofline"] and line["roofline"]["peak_measured_stream_read"] is None
    frame = np.load(str(tmp_path / "frame.npy"))
    assert frame.shape == (368, 640, 4) and np.isfinite(frame).all()


@pytest.mark.gpu
def test_a_plain_run_still_checks_the_frame_when_asked():
    """--check 1 without --full: the bit-exact kernel variant, every pass played replayed by the CPU oracle on a band of rows"""
    line = _run_bench(["--check", "1", "--fast-math", "0", "--warmup-seconds", "0"])
    assert line["frame_check"] is True and "bit-identical" in line["frame_check_kind"]
    assert "other_configs" not in line and "cpu_baseline" not in line
