"""Every asynchronous entry point in stream order on a caller's stream (vpt_context_create_on_stream, VPT_OPTION_SPLIT_STREAMS).

The work runs in tests/stream_order_worker.py, in ONE fresh process (the consumer is torch work on torch's stream, and a
GPU-initialised torch stays out of this process).  Each scenario there runs as a synchronised twin, as a twin on stale inputs and in
stream order behind a delay kernel, with no host synchronisation; one test here per scenario asserts its line:

  * the ordered run's bytes equal the synchronised twin's (the message names the first differing byte),
  * the twin on stale inputs differs in at least 1 % of the bytes (so stale inputs or a stale image cannot pass),
  * in a scenario marked asynchronous the gate was still closed when the last library call returned (no entry waited for the host).

DESIGN.md section 6 ("Stream order on a caller's stream") holds the scenario families, the measured gate and the mutation table."""
import json
import os
import subprocess
import sys

import pytest

from stream_order_worker import SCENARIOS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def worker():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_order_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    out = p.stdout.decode(errors="replace")
    lines = {}
    for line in out.splitlines():
        f = line.split("\t")
        if len(f) == 4 and f[0] == "RESULT":
            lines[f[1]] = (f[2], json.loads(f[3]))
    return p.returncode, lines, out


@pytest.mark.parametrize("name", [s["name"] for s in SCENARIOS])
def test_stream_order(worker, name):
    code, lines, out = worker
    assert name in lines, "the worker (exit code %d) has no line for this scenario; its output ends:\n%s" % (code, out[-3000:])
    status, rep = lines[name]
    what = "%s: %s\n  first difference: %s\n  stale twin differs in %.2f %% of the bytes\n  gate: %s (%s; enqueued in %s ms, gate %s ms)" % (
        name, "; ".join(rep.get("problems", [])) or "ok", rep.get("first_difference"), 100.0 * rep.get("stale_fraction", 0.0),
        rep.get("gate"), rep.get("waits"), rep.get("enqueue_ms"), rep.get("gate_ms"))
    assert status == "PASS", what + ("\n" + rep["traceback"] if "traceback" in rep else "")
    assert rep["first_difference"] is None and rep["stale_fraction"] >= 0.01, what
    if rep["waits"] == "asynchronous":
        assert rep["gate"] == "closed", what


def test_worker_ran_every_scenario_and_left_cleanly(worker):
    code, lines, out = worker
    assert code == 0 and set(lines) == {s["name"] for s in SCENARIOS}, out[-3000:]
