"""GPU: bench.py's plain line (the headline only) and --dump-outputs (what the last timed pass computed, the same from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--loci", "300",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_outputs(tmp_path):
    a = _bench(tmp_path / "a", 3)
    assert a["steps"] == 3 and a["n_gpus"] == 1 and a["higher_is_better"] is True and a["dtype"] == "f64"
    assert abs(a["value"] - 300 / (a["ms_per_step"] * 1e-3)) < 1e-6 * a["value"]
    for moved in ("roofline", "value_one_in_flight", "value_incl_h2d", "extra", "cpu_baseline"):
        assert moved not in a, moved
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in ("units", "mode_genotype", "spm_gpm", "n_genotypes", "mode_count", "trace_units",
                                                "trace_genotypes", "trace_llks"))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    arrays = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(x.dtype in (np.float32, np.float64) for x in arrays.values())
    assert arrays["mode_genotype.npy"].shape == (300, 4, 8) and arrays["trace_genotypes.npy"].shape == (64, 2, 1000, 4, 8)
    assert ((arrays["spm_gpm.npy"] > 0) & (arrays["spm_gpm.npy"] <= 1)).all()
    # another run with the same arguments but another number of steps hands the caller the same arrays
    _bench(tmp_path / "b", 2)
    for n in names:
        assert np.array_equal(arrays[n], np.load(tmp_path / "b" / n)), n
