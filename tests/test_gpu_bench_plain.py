"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` run at a small size:
the result line holds the headline figures and none of --full's lines, --steps sets the timed
steps, and the dumped arrays are the MSM of the bench's seeded inputs (bases seed 2024, scalars
default_rng(1234)) as the C oracle computes it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_N = 10


def test_plain_run_line_and_dump(oracle_c, tmp_path):
    import vkzg
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--log-n", str(LOG_N), "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == 3 and j["warmup"] == 1 and j["n_gpus"] == 1 and j["full"] is False
    assert j["ms_per_step"] > 0 and abs(j["value"] * j["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert j["config"]["n_points"] == 1 << LOG_N
    for k in ("roofline", "kernel_ms", "result_check", "variable_base", "host_scalars", "secondary", "kzg",
              "multiproof", "ipa", "verkle", "cpu_baseline"):
        assert k not in j, k
    assert sorted(os.listdir(out)) == ["msm_inf.npy", "msm_xy_u16.npy"]
    words, inf = np.load(out / "msm_xy_u16.npy"), np.load(out / "msm_inf.npy")
    assert words.dtype == np.float64 and inf.dtype == np.float64
    got = words.astype("<u2").view("<u8")
    # the same inputs, rebuilt here: the bench's seeds
    n = 1 << LOG_N
    e = vkzg.Engine("bls12_381")
    try:
        xy, binf = e.download_bases(e.random_bases(n, seed=2024))
    finally:
        e.close()
    sc = vkzg.random_scalars("bls12_381", n, np.random.default_rng(1234))
    want, winf = oracle_c.msm_arrays("bls12_381", xy, binf, sc, 8)
    assert int(inf[0]) == winf == j["result_inf"]
    assert np.array_equal(got, np.asarray(want, dtype=np.uint64))
