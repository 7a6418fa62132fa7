"""bench.py on one GPU: a plain run reports the headline from the set-up and the timed steps alone; --full adds the figures
that take work of their own (instrumented cycle, residual, F-cycles, other restriction setting, cycle without events,
cpu_baseline) and leaves the timed steps and what --dump-outputs writes as they are.  -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("ms_per_step_without_events", "other_restriction_setting", "fcycle_ms", "spmv_finest", "events_ms",
             "events_petsc_names", "events_note", "rel_residual_after_timed_cycles")


def _bench(args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ALFI_DIST_FORCE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny"] + args,
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.returncode, out.stdout[-2000:], out.stderr[-3000:])
    return json.loads(lines[0])


def test_plain_and_full_runs(tmp_path):
    plain = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain")])
    full = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "full"), "--full"])
    for d in (plain, full):
        assert all(k in d for k in HEADLINE), sorted(d)
        assert d["unit"] == "V-cycles/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
        assert d["roofline"]["launches"] > 0 and d["roofline"]["achieved"] > 0
    assert not [k for k in FULL_ONLY if k in plain], sorted(plain)
    assert plain["cpu_baseline"]["value"] is None
    assert all(k in full for k in FULL_ONLY), sorted(full)
    assert full["rel_residual_after_timed_cycles"] < 0.5
    assert full["fcycle_ms"] > 0 and full["other_restriction_setting"]["ms_per_step"] > 0
    assert full["events_ms"]["MATMULT"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["kind"] == "port"
    # the timed steps compute the same iterate either way
    xp, xf = np.load(tmp_path / "plain" / "x.npy"), np.load(tmp_path / "full" / "x.npy")
    assert xp.shape == xf.shape and np.abs(xp - xf).max() <= 1e-10 * np.abs(xf).max()


def test_full_without_cpu_baseline():
    d = _bench(["--steps", "2", "--warmup", "0", "--full", "--no-cpu-baseline"])
    assert all(k in d for k in FULL_ONLY), sorted(d)
    assert d["cpu_baseline"]["value"] is None and d["cpu_baseline"]["sample"] == "skipped"
