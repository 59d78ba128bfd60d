"""bench.py on the device: a plain run measures the headline and nothing else; --full adds the checks and the per-kernel figures
without changing what the timed path computes."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "3", "--reps", "2", "--batch", "2", "--seconds", "1", "--prompt-frames", "24"]


def _run(args, tmp_path, tag):
    detail = tmp_path / f"{tag}.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args + ["--detail-json", str(detail),
                       "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return lines, json.load(open(detail)), np.load(tmp_path / tag / "latent.npy")


def test_bench_plain_run_is_lean_and_full_adds_the_checks(tmp_path):
    lines, rec, y = _run([], tmp_path, "plain")
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 3 and d["dtype"] == "fp16" and d["finite"]
    assert d["value"] == pytest.approx(3e3 / (d["ms_per_step"] * 3), rel=1e-4)
    for k in ("roofline", "parity", "cpu_baseline", "graph_equals_eager"):
        assert d[k] is None, k
    assert rec["loop_check"] is None and rec["attention_fallback_workgroups"] is None and rec["gn_prologue_workgroups_alone"] is None

    lines_f, rec_f, y_f = _run(["--full", "--skip-cpu", "--skip-fp32", "--skip-others", "--skip-strong"], tmp_path, "full")
    assert len(lines_f) == 2 and lines_f[0] == lines_f[1]
    f = json.loads(lines_f[-1])
    assert f["graph_equals_eager"] is True and f["roofline"]["bound"] == "mfma" and 0 < f["roofline"]["frac"] < 1
    assert rec_f["attention_fallback_workgroups"] is not None and rec_f["gn_prologue_workgroups_alone"] is not None
    # what the timed path returns does not depend on --full
    assert y.shape == (2, 100, 94) and np.isfinite(y).all() and np.array_equal(y, y_f)
