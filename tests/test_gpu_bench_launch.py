"""bench.py's N > 1 path on the one-GPU box.

  * ``python bench.py --gpus 2`` with one visible GPU exits 2 without a bench line;
  * ``--gpus 2 --one-device-rehearsal --full`` launches two ranks through torch.distributed.run
    (this script's own launcher), both on cuda:0 over gloo, and runs the whole N > 1 bench —
    sharded-panel search, timed steps, max-over-ranks timing, the 2-rank training leg with
    the panel sharded 2-way and the bucketed gradient all-reduce — at a small size.  The
    numbers are not a measurement; the test checks the line's world size and shape;
  * a plain ``--gpus 1`` run (in this process, at a small size) times exactly ``--steps``
    steps, prints the headline line without the ``--full`` legs, and with ``--dump-outputs``
    writes the last step's outputs, the same from run to run.
"""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}


@pytest.mark.timeout(200)
def test_bench_more_gpus_than_visible_fails_loudly():
    n = torch.cuda.device_count()
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", str(n + 1), "--steps", "1"],
                       capture_output=True, text=True, timeout=180, env=_env(), cwd=str(REPO))
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert f"needs {n + 1} visible GPUs, found {n}" in r.stderr
    assert '"n_gpus"' not in r.stdout


@pytest.mark.timeout(400)
def test_bench_two_rank_rehearsal_on_one_gpu():
    cmd = [sys.executable, "-u", str(REPO / "bench.py"), "--gpus", "2", "--one-device-rehearsal", "--full",
           "--n-ref", "20000", "--batch", "4", "--layers", "2", "--steps", "2", "--warmup", "1",
           "--f32-leg", "0", "--c2-n", "0", "--train-steps", "1", "--cpu-baseline", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=380, env=_env(), cwd=str(REPO))
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = lines[0]
    assert line["n_gpus"] == 2
    assert line["distributed"] == {"backend": "gloo", "world_size": 2, "rehearsal_one_device": True}
    assert line["config"]["global_batch"] == 8
    assert "panel sharded 2-way" in line["config"]["parallelism"]
    assert line["masked_snvs_per_step_per_gpu"] > 0 and line["value"] > 0
    assert line["train"]["n_gpus"] == 2 and line["train"]["panel"] == "sharded 2-way"
    assert line["cpu_baseline"] is None


def test_plain_run_is_lean_and_dumps_repeatable_outputs(tmp_path, monkeypatch, capsys):
    """Two plain runs with the same arguments: 1 warm-up + 3 timed calls of the step each, a
    line with the headline keys and none of the ``--full`` legs, and the same dump.  The inputs
    the step echoes (af, af_p) and the embedded block (integer neighbour counts) must be equal
    bit for bit; the probabilities within 1e-2, two bf16 ulps at 1.0 (2 * 2^-8 = 7.8e-3)
    for kernels whose accumulation order may differ between launches."""
    import numpy as np
    import bench
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        monkeypatch.delenv(v, raising=False)
    calls = []
    make_step = bench.make_step

    def counting(wl, eng, k):
        step = make_step(wl, eng, k)
        return lambda: calls.append(1) or step()
    monkeypatch.setattr(bench, "make_step", counting)
    dumps = []
    for name in ("a", "b"):
        del calls[:]
        bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--n-ref", "20000", "--batch", "4",
                    "--layers", "2", "--dump-outputs", str(tmp_path / name)])
        assert len(calls) == 4
        lines = [json.loads(s) for s in capsys.readouterr().out.splitlines() if s.startswith("{")]
        assert len(lines) == 1
        line = lines[0]
        assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
        assert line["unit"] == "masked SNVs/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
        assert line["ms_per_step"] > 0
        assert abs(line["value"] - line["masked_snvs_per_step_per_gpu"] / (line["ms_per_step"] * 1e-3)) \
            <= 1e-3 * line["value"]
        for moved in ("cpu_baseline", "precision_parity", "train"):
            assert moved not in line
        for moved in ("knn_hbm_probe", "knn_c2_embedding_space", "knn_search_ms"):
            assert moved not in line["kernels"]
        dumps.append({p.stem: np.load(p) for p in sorted((tmp_path / name).iterdir())})
    a, b = dumps
    assert sorted(a) == sorted(b) == ["af", "af_p", "gt", "h1_after", "h1_before", "h2_after", "h2_before",
                                      "probs_h1", "probs_h2"]
    assert a["probs_h1"].shape == (4, 1030, 2) and a["h1_after"].shape == (4, 1030, 384)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for key in a:
        assert a[key].dtype == np.float32 and np.isfinite(a[key]).all()
    for key in ("af", "af_p", "h1_before", "h2_before"):
        np.testing.assert_array_equal(a[key], b[key])
    for key in ("probs_h1", "probs_h2", "gt"):
        np.testing.assert_allclose(a[key], b[key], rtol=0, atol=1e-2)
