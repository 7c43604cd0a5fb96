"""The opt-in device VCF writer (csrc/vcf.hip ``snvrag_vcf_format``, src/vcf_device.py
``write_vcf_device``, ``--vcf_writer device``) against the unchanged host ``write_vcf``: the files
are compared as bytes.  Sample counts straddle the kernel's 256-cell tile, prefix lengths cover every
destination alignment modulo 16, and the values are the '%.3f' rounding boundaries of
test_vcf_writer_cpu.py."""
import functools
import os

import numpy as np
import pytest
import torch

from test_vcf_writer_cpu import boundary_values

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N_SITES = 40
CHROM = "21"


@functools.lru_cache(maxsize=None)
def case(S):
    """40 sites x S samples: inputs (read-only) and the host writer's file, computed once per S."""
    rng = np.random.default_rng(100 + S)
    pool = boundary_values()
    small = pool[pool <= np.nextafter(np.float32(2), np.float32(3))]      # gp1, ds stay far below 9.9995
    n = N_SITES
    h1, h2 = rng.choice(pool, (n, S)), rng.choice(pool, (n, S))
    gt = rng.choice(small, (n, S, 4))
    gt[::3, :, 0] = rng.choice(pool, gt[::3, :, 0].shape)                 # 9.9994 reaches gp0 too
    for r in (3, 17, 39):                                                 # sites no window covers: all zero
        h1[r], h2[r], gt[r] = 0, 0, 0
    gt[5] = 0.25                                                          # exact argmax ties: the first wins
    gt[6] = np.float32([0, 0.5, 0.5, 0])
    gt[7, :, 1], gt[7, :, 2] = np.float32(0.1), np.float32(0.7)          # gt[1] + gt[2] rounds in f32
    assert float(gt[7, 0, 1]) + float(gt[7, 0, 2]) != float(gt[7, 0, 1] + gt[7, 0, 2])
    gt[8] = rng.random((S, 4), dtype=np.float32) / 4                      # ordinary probabilities
    h1[8], h2[8] = rng.random(S, dtype=np.float32), rng.random(S, dtype=np.float32)
    pos = np.asarray([10 ** (4 * (i // 16)) + i % 7 for i in range(n)], np.int64)   # 1, 5 and 9 digits
    ref = [("ACGT" * 4)[:1 + i % 16] for i in range(n)]                   # 16 consecutive prefix lengths per group
    alt = ["GA" if i in (16, 17) else "T" for i in range(n)]              # shifts the later lines: all 16 alignments
    samples = [f"S{i}" for i in range(S)]
    for a in (h1, h2, gt):
        assert a.dtype == np.float32
        a.setflags(write=False)
    return dict(h1=h1, h2=h2, gt=gt, pos=pos, ref=ref, alt=alt, samples=samples)


def host_bytes(tmp_path, c, name="host.vcf", **kw):
    from src.infer_embedding_rag import write_vcf
    kw = {**dict(ref=c["ref"], alt=c["alt"]), **kw}
    write_vcf(tmp_path / name, CHROM, c["pos"], c["h1"], c["h2"], c["gt"], c["samples"], **kw)
    return (tmp_path / name).read_bytes()


def device_bytes(tmp_path, c, form="device", name="dev.vcf", expect=True, **kw):
    from src.infer_embedding_rag import write_vcf_device
    conv = {"device": lambda a: torch.from_numpy(a.copy()).to(DEV), "host": lambda a: torch.from_numpy(a.copy()),
            "numpy": lambda a: a}[form]
    kw = {**dict(ref=c["ref"], alt=c["alt"], device=DEV), **kw}
    ok = write_vcf_device(tmp_path / name, CHROM, c["pos"], conv(c["h1"]), conv(c["h2"]), conv(c["gt"]),
                          c["samples"], **kw)
    assert ok is expect
    return (tmp_path / name).read_bytes()


def first_difference(a, b):
    if a == b:
        return None
    i = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
    return len(a), len(b), i, a[max(0, i - 45):i + 45], b[max(0, i - 45):i + 45]


@pytest.mark.parametrize("S", [1, 2, 255, 256, 257, 700])
def test_file_equals_host_writer_bytes(tmp_path, S):
    from src import vcf_device as V
    c = case(S)
    want = host_bytes(tmp_path, c)
    got = device_bytes(tmp_path, c)
    assert first_difference(got, want) is None
    # what the inputs set out to cover: 16 consecutive prefix lengths, and every alignment modulo 16
    # of a line body's first byte in the chunk buffer
    _, _, p_off = V.site_prefixes(CHROM, c["pos"], None, c["ref"], c["alt"])
    plen = np.diff(p_off)
    assert set(range(int(plen.min()), int(plen.min()) + 16)) <= set(plen.tolist())
    starts = np.concatenate([[0], np.cumsum(V.line_lengths(p_off, S))])[:-1] + plen
    assert len(set((starts % 16).tolist())) == 16


@pytest.mark.parametrize("S", [257])
def test_chunking_gives_the_one_chunk_file(tmp_path, S):
    from src import vcf_device as V
    c = case(S)
    want = host_bytes(tmp_path, c)
    _, _, p_off = V.site_prefixes(CHROM, c["pos"], None, c["ref"], c["alt"])
    length = V.line_lengths(p_off, S)
    three = int(max(length[i:i + 3].sum() for i in range(len(length) - 2)))
    assert all(hi - lo == 3 for lo, hi in V.plan_chunks(length, three)[:-1])
    assert all(hi - lo == 1 for lo, hi in V.plan_chunks(length, int(length.max())))
    for cb in (three, int(length.max())):
        assert first_difference(device_bytes(tmp_path, c, chunk_bytes=cb), want) is None
        assert first_difference(device_bytes(tmp_path, c, form="numpy", chunk_bytes=cb), want) is None
    with pytest.raises(ValueError, match="does not fit"):
        device_bytes(tmp_path, c, chunk_bytes=int(length.max()) - 1)
    with pytest.raises(ValueError, match="1 GiB"):
        device_bytes(tmp_path, c, chunk_bytes=(1 << 30) + 1)


@pytest.mark.parametrize("pattern", ["none", "all", "mixed"])
def test_pos_flag_selects_what_the_host_writer_selects(tmp_path, pattern):
    c = case(3)
    flag = {"none": np.zeros(N_SITES, bool), "all": np.ones(N_SITES, bool),
            "mixed": np.random.default_rng(5).random(N_SITES) < 0.4}[pattern]
    want = host_bytes(tmp_path, c, pos_flag=flag)
    if pattern == "none":
        assert want.count(b"\n") == 7 and want.endswith(b"\tS0\tS1\tS2\n")       # the header only
    for form in ("device", "numpy"):
        assert first_difference(device_bytes(tmp_path, c, form=form, pos_flag=flag), want) is None
    got = device_bytes(tmp_path, c, pos_flag=torch.from_numpy(flag).to(DEV), ref=None, alt=None)
    assert first_difference(got, host_bytes(tmp_path, c, pos_flag=flag, ref=None, alt=None)) is None


def test_input_forms_give_the_same_bytes(tmp_path):
    c = case(70)
    want = host_bytes(tmp_path, c)
    for form in ("device", "host", "numpy"):
        assert first_difference(device_bytes(tmp_path, c, form=form, name=f"{form}.vcf"), want) is None
    with pytest.raises(TypeError, match="float32"):
        device_bytes(tmp_path, dict(c, h1=c["h1"].astype(np.float64)), form="numpy")


@pytest.mark.parametrize("form", ["device", "numpy"])
@pytest.mark.parametrize("what", ["nan", "negzero", "ten", "nan_last_chunk"])
def test_values_that_do_not_fit_fall_back_to_the_host_writer(tmp_path, capsys, what, form):
    """An ordinary data path: the kernel counts the value and formats on; the writer reads the count
    before the chunk's bytes reach the file, discards the partial file and runs ``write_vcf``."""
    base = case(70)
    c = dict(base, h1=base["h1"].copy(), h2=base["h2"].copy(), gt=base["gt"].copy())
    kw = {}
    if what == "nan":
        c["h1"][11, 40] = np.nan
    elif what == "negzero":
        c["gt"][20, 69, 3] = -0.0               # gp2 is printed as it stands: the host writes -0.000
    elif what == "ten":
        c["h2"][0, 0] = 10.0
    else:                                       # one line per chunk: 39 chunks are on disk when the 40th fails
        from src import vcf_device as V
        _, _, p_off = V.site_prefixes(CHROM, c["pos"], None, c["ref"], c["alt"])
        c["gt"][N_SITES - 1, 3, 0] = np.nan
        kw["chunk_bytes"] = int(V.line_lengths(p_off, 70).max())
    out = tmp_path / "out"
    out.mkdir()
    want = host_bytes(tmp_path, c)
    got = device_bytes(out, c, form=form, expect=False, **kw)
    assert first_difference(got, want) is None
    assert os.listdir(out) == ["dev.vcf"]       # no partial or temporary file is left
    note = capsys.readouterr().out
    assert note.count("\n") == 1 and "host writer" in note


def test_kernel_refuses_bad_arguments_and_skips_broken_lines():
    """The entry point's argument checks, and the kernel's own guard: a line whose offsets break the
    contract (length != prefix + 40 S, a row outside the arrays) is counted and left unwritten."""
    from src import kernels as K
    S, n = 5, 3
    h1, h2 = torch.rand(n, S, device=DEV), torch.rand(n, S, device=DEV)
    gt = torch.rand(n, S, 4, device=DEV) / 4
    prefix = torch.frombuffer(bytearray(b"ab\tcde\t"), dtype=torch.uint8).to(DEV)
    p_off = torch.tensor([0, 3, 7], dtype=torch.int32, device=DEV)
    good = torch.tensor([0, 3 + 40 * S, 7 + 80 * S], dtype=torch.int64, device=DEV)
    rows = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    nbytes = 7 + 80 * S
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)

    def run(rows=rows, line_off=good, out_bytes=nbytes, out=None):
        out = torch.full((nbytes + 64,), 0x7e, dtype=torch.uint8, device=DEV) if out is None else out
        bad.zero_()
        K.vcf_format(h1, h2, gt, rows, line_off, p_off, prefix, out, out_bytes, bad)
        return bytes(out.cpu().numpy()), int(bad.item())

    text, count = run()
    assert count == 0 and text[nbytes:] == b"~" * 64
    assert text.startswith(b"ab\t") and text[3 + 40 * S - 1:3 + 40 * S + 4] == b"\ncde\t" and text[nbytes - 1:nbytes] == b"\n"
    assert text[:nbytes].count(b"\t") == 2 * (S - 1) + 2 and text[:nbytes].count(b":") == 2 * S * 3
    text, count = run(line_off=good + torch.tensor([0, 1, 1], device=DEV), out_bytes=nbytes + 1)   # line 0 too long
    assert count == 1 and text[:3 + 40 * S + 1] == b"~" * (3 + 40 * S + 1) and text[nbytes + 1:] == b"~" * 63
    assert text[3 + 40 * S + 1:].startswith(b"cde\t") and text[nbytes:nbytes + 1] == b"\n"
    text, count = run(rows=torch.tensor([n, -1], dtype=torch.int32, device=DEV))    # rows outside [0, n)
    assert count == 2 and text == b"~" * (nbytes + 64)
    text, count = run(out_bytes=nbytes - 1)                                         # last line past the chunk's end
    assert count == 1 and text[3 + 40 * S:] == b"~" * (4 + 40 * S + 64)
    for kw, msg in ((dict(out=torch.zeros(nbytes + 64, dtype=torch.uint8, device=DEV)[1:]), "aligned"),
                    (dict(out_bytes=40 * S), "exceed the chunk")):
        with pytest.raises(RuntimeError, match=msg):
            run(**kw)


@pytest.mark.parametrize("device_features", [False, True])
def test_infer_cli_device_writer_writes_the_host_writers_file(tmp_path, monkeypatch, device_features):
    """``--vcf_writer device`` through the entry point: imputed.vcf byte-identical to the host writer's
    run, imputed.npz unchanged; with ``--device_features`` the writer formats in place from the scatter
    path's device arrays (``site_dev``), without it from the host arrays through the upload path."""
    from src import infer_embedding_rag as I
    seen = []
    real = I.write_vcf_device

    def spy(path, chrom, pos, h1, h2, gt, *a, **kw):
        seen.append(all(torch.is_tensor(t) and t.is_cuda for t in (h1, h2, gt)))
        ok = real(path, chrom, pos, h1, h2, gt, *a, **kw)
        seen.append(ok)
        return ok

    monkeypatch.setattr(I, "write_vcf_device", spy)
    args = ["--synthetic", "6", "--synthetic_sites", "2040", "--synthetic_ref", "24", "-d", "64", "-l", "2", "-a", "2",
            "-b", "4", "--k_retrieve", "3", "--mask_rate", "0.5", "--index_window_len", "1020"]
    args += ["--device_features"] if device_features else []
    res_h = I.infer(args + ["--vcf_writer", "host", "-o", str(tmp_path / "host")])
    assert seen == []
    res_d = I.infer(args + ["--vcf_writer", "device", "-o", str(tmp_path / "device")])
    assert seen == [device_features, True]
    assert "site_dev" not in res_h and "site_dev" not in res_d
    a, b = (tmp_path / "device" / "imputed.vcf").read_bytes(), (tmp_path / "host" / "imputed.vcf").read_bytes()
    assert b.count(b"\n") > 7 + 500                       # about half of the 2040 sites are imputed
    assert first_difference(a, b) is None
    za, zb = np.load(tmp_path / "device" / "imputed.npz"), np.load(tmp_path / "host" / "imputed.npz")
    assert za.files == zb.files
    for k in zb.files:
        assert np.array_equal(za[k], zb[k]), k
