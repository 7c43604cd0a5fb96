"""bench.py's ``--full`` / ``--dump-outputs`` options and the output dump, on the CPU:

  * a plain command line leaves ``--full`` off and writes no dump; ``--steps`` below 1 is refused;
  * ``dump_outputs`` writes every tensor of the step's dict as float32 ``<name>.npy``: small
    ones whole, large ones as the same seeded, ascending sample of rows in every call; the
    non-tensor entries and ``x_all`` (h1_after and h2_after are its halves) are left out;
  * the dump of the benchmarked shape stays under the 64 MB limit.
"""

import numpy as np
import pytest
import torch


def _bench():
    import bench
    return bench


def test_plain_command_line_is_lean():
    b = _bench()
    args = b.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert args.full is False and args.dump_outputs is None
    assert args.steps == 7 and args.warmup == 3
    args = b.parse(["--full", "--dump-outputs", "some/dir"])
    assert args.full is True and args.dump_outputs == "some/dir"
    with pytest.raises(SystemExit):
        b.parse(["--steps", "0"])


def _step_dict(rows):
    g = torch.Generator().manual_seed(5)
    xx = torch.randn(2 * rows, 384, generator=g).to(torch.bfloat16)
    return dict(h1_after=xx[:rows], h2_after=xx[rows:], x_all=xx, B=4, L=rows // 4,
                probs_h1=torch.rand(4, rows // 4, 2, generator=g), gt=torch.rand(4, rows // 4, 3, generator=g),
                af=torch.rand(4, rows // 4, generator=g))


def test_dump_outputs_writes_float32_arrays(tmp_path):
    b = _bench()
    rows = 4 * 1500                                   # 6000 x 384 f32 = 9.2 MB > DUMP_FULL_BYTES: sampled
    out = _step_dict(rows)
    assert out["h1_after"].numel() * 4 > b.DUMP_FULL_BYTES
    b.dump_outputs(out, tmp_path / "a")
    b.dump_outputs(out, tmp_path / "b")
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["af.npy", "gt.npy", "h1_after.npy", "h2_after.npy", "probs_h1.npy"]
    for n in names:
        a, a2 = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32
        np.testing.assert_array_equal(a, a2)
    # small outputs whole, bit for bit
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "gt.npy"), out["gt"].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "af.npy"), out["af"].numpy())
    # large outputs: DUMP_SAMPLE_ROWS distinct rows of the [-1, D] view, in ascending order
    h = np.load(tmp_path / "a" / "h2_after.npy")
    assert h.shape == (b.DUMP_SAMPLE_ROWS, 384)
    full = out["h2_after"].float().numpy()
    rows_of = {r.tobytes(): i for i, r in enumerate(full)}
    picked = [rows_of[r.tobytes()] for r in h]
    assert picked == sorted(set(picked))


def test_dump_of_the_benchmarked_shape_fits_the_limit():
    """configs[2]: B = 256, L = 1030, D = 384.  Whole: probs 2 x B*L*2, gt B*L*4 at most, af and
    af_p B*L each; sampled: the four hidden states."""
    b = _bench()
    B, L, D = 256, 1030, 384
    assert B * L * 4 * 4 <= b.DUMP_FULL_BYTES < B * L * D * 4
    whole = 4 * (2 * B * L * 2 + B * L * 4 + 2 * B * L)
    sampled = 4 * (4 * b.DUMP_SAMPLE_ROWS * D)
    assert whole + sampled <= b.DUMP_LIMIT_BYTES == 64 << 20
