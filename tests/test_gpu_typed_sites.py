"""GPU tests of the typed-site overlay (csrc/typed.hip ``snvrag_typed_overlay``, ``typed_sites.typed_overlay``,
``--vcf_sites all``): the kernel against the numpy specification bit for bit at its tile edges (64 site rows x 64
columns per workgroup), with guard rows around every output; the chunked host-array path; refused calls; and the
entry point end to end on synthetic data, with both writers, with and without the device result arrays, with
INFO / BGZF / index, and with a VCF target that holds missing calls.

The end-to-end runs use 1320 synthetic sites: synthetic datasets are cut into the fixed 1020-site windows, so this
is the smallest run with two windows and a ragged last one (300 sites).
"""
import ctypes as C
import gzip

import numpy as np
import pytest
import torch

from test_typed_sites_cpu import CELL, NAN_PATTERN, nan_fill, random_bits, same_bits

from src import kernels as K
from src import native
from src import typed_sites as T
from src.dataset import vcf_reader as V

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
GUARD = 3                                        # guard rows in front of and behind every output array


# ------------------------------------------------------------------------------------------------ the kernel --
def make_case(seed, n, S, n_target, rows="random", miss="scattered", permuted=False, extra_ld=0):
    rng = np.random.default_rng([seed, n, S, n_target])
    S_target = S + 3 if permuted else S
    ld = (n_target + 7) // 8 + extra_ld
    alt, ms = random_bits(rng, S_target, n_target, max(ld, 1), miss_rate={"scattered": 0.1, "none": 0.0}.get(miss, 0.02))
    if miss == "site":                           # a whole record
        r = n_target - 1
        ms[:, r >> 3] |= np.uint8(1 << (r & 7))
    if miss == "sample":                         # a whole sample (both haplotypes)
        ms[2 * (S_target // 2):2 * (S_target // 2) + 2] = 0xff
    if rows == "random":
        site_row = rng.integers(0, n_target, n)
        site_row[rng.random(n) < 0.3] = -1
        site_row[rng.integers(0, n)] = n_target - 1          # the last record
        if n > 2:
            site_row[1], site_row[2] = n_target, -5          # out of range
    elif rows == "none":
        site_row = np.full(n, -1)
    elif rows == "equal":
        site_row = np.full(n, n_target - 1)
    else:                                        # monotone with gaps (repeats where n_target is small), or reversed
        site_row = np.sort(rng.integers(0, n_target, n))
        site_row[rng.random(n) < 0.25] = -1
        if rows == "reversed":
            site_row = site_row[::-1]
    col = np.arange(S)
    if permuted:
        col = rng.permutation(S_target)[:S]
        if S > 1:
            col[S // 2] = -1
        if S > 2:
            col[0] = S_target                    # out of range
    return dict(n=n, S=S, n_target=n_target, alt=alt, miss=ms, site_row=site_row.astype(np.int32),
                col=col.astype(np.int32))


def run_case(c):
    """The kernel on guarded device buffers against the specification on host copies: every byte of the buffers,
    guard rows included.  Returns ``missing``."""
    n, S = c["n"], c["S"]
    host = [nan_fill((n + 2 * GUARD, S)), nan_fill((n + 2 * GUARD, S)), nan_fill((n + 2 * GUARD, S, 4))]
    m_host = np.full(n + 2 * GUARD, -7, np.int32)
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    m_dev = torch.from_numpy(m_host).to(DEV)
    up = lambda a: torch.from_numpy(a).to(DEV)
    got = K.typed_overlay(*(d[GUARD:GUARD + n] for d in dev), up(c["alt"]), up(c["miss"]), c["n_target"],
                          up(c["site_row"]), up(c["col"]), missing=m_dev[GUARD:GUARD + n])
    torch.cuda.synchronize()
    want = T.typed_overlay_host(*(a[GUARD:GUARD + n] for a in host), c["alt"], c["miss"], c["n_target"], c["site_row"],
                                c["col"])
    m_host[GUARD:GUARD + n] = want
    for d, a, name in zip(dev, host, ("h1", "h2", "gt")):
        assert same_bits(d.cpu().numpy(), a), name
    assert np.array_equal(m_dev.cpu().numpy(), m_host)
    assert np.array_equal(got.cpu().numpy(), want)
    return want


N_TARGETS = [1, 8, 9, 63, 64, 65, 1000]


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130, 257])
@pytest.mark.parametrize("n", [1, 7, 64, 65, 200])
def test_kernel_equals_the_specification(n, S):
    # every (n, S) with two record counts, so that each n_target meets small and large shapes
    k = [1, 7, 64, 65, 200].index(n) * 6 + [1, 63, 64, 65, 130, 257].index(S)
    for j in (k, k + 3):
        run_case(make_case(1, n, S, N_TARGETS[j % 7]))


@pytest.mark.parametrize("n_target", N_TARGETS)
def test_kernel_last_record_and_padded_rows(n_target):
    """Every row maps the last record (bit (n_target - 1) & 7 of the last byte: bit 7 at 8, 64 and 1000), in bit
    rows wider than needed and with S != S_target through a permuted ``col``."""
    c = make_case(2, 70, 67, n_target, rows="equal", permuted=True, extra_ld=5)
    m = run_case(c)
    assert c["alt"].shape == (2 * 70, (n_target + 7) // 8 + 5)
    r = n_target - 1
    cols = c["col"][(c["col"] >= 0) & (c["col"] < 70)]
    bit = lambda b, row: (b[row, r >> 3] >> (r & 7)) & 1
    assert (m == int((bit(c["miss"], 2 * cols) | bit(c["miss"], 2 * cols + 1)).sum())).all()


@pytest.mark.parametrize("rows", ["none", "monotone", "reversed", "equal"])
@pytest.mark.parametrize("permuted", [False, True])
def test_kernel_site_row_orders(rows, permuted):
    m = run_case(make_case(3, 200, 130, 1000, rows=rows, permuted=permuted, extra_ld=3))
    if rows == "none":
        assert not m.any()                       # nothing written (run_case compared every byte), missing all 0


@pytest.mark.parametrize("miss", ["site", "sample", "scattered", "none"])
def test_kernel_missing_calls(miss):
    c = make_case(4, 65, 65, 64, rows="monotone", miss=miss)
    c["site_row"][10] = 63
    m = run_case(c)
    if miss == "site":
        assert m[10] == 65 and (m[c["site_row"] == 63] == 65).all()          # the whole row stays the model's
    if miss == "sample":
        assert (m[c["site_row"] >= 0] >= 1).all()
    if miss == "none":
        assert not m.any()
    if miss == "scattered":
        assert 0 < m.sum() < 65 * 65


def test_kernel_no_rows():
    lib = native.load()
    buf = torch.zeros(1024, device=DEV, dtype=torch.uint8)
    p = buf.data_ptr()
    assert lib.snvrag_typed_overlay(p, p, 8, 10, 2, p, p, 0, 2, p, p, p, p, None) == 0
    e = torch.empty(0, 4, device=DEV)
    m = K.typed_overlay(e, e.clone(), torch.empty(0, 4, 4, device=DEV), buf[:16].view(4, 4), buf[16:32].view(4, 4), 10,
                        torch.empty(0, device=DEV, dtype=torch.int32), torch.zeros(4, device=DEV, dtype=torch.int32))
    assert m.shape == (0,)


def test_refused_calls_change_nothing():
    lib = native.load()
    fill = 0xA5
    bufs = [torch.full((4096,), fill, dtype=torch.uint8, device=DEV) for _ in range(8)]
    alt, ms, row, col, h1, h2, gt, missing = (b.data_ptr() for b in bufs)

    def call(**kw):
        a = dict(alt=alt, ms=ms, ld=2, n_target=16, S_target=2, row=row, col=col, n=4, S=2, h1=h1, h2=h2, gt=gt,
                 missing=missing)
        a.update(kw)
        rc = lib.snvrag_typed_overlay(a["alt"], a["ms"], a["ld"], a["n_target"], a["S_target"], a["row"], a["col"],
                                      a["n"], a["S"], a["h1"], a["h2"], a["gt"], a["missing"], None)
        return rc, lib.snvrag_last_error().decode()

    cases = [dict(alt=None), dict(ms=None), dict(row=None), dict(col=None), dict(h1=None), dict(h2=None), dict(gt=None),
             dict(missing=None), dict(gt=gt + 4), dict(h1=h1 + 2), dict(missing=missing + 1), dict(ld=1), dict(S=0),
             dict(S_target=0), dict(S=1 << 29), dict(n=-1), dict(n_target=-1), dict(n=1 << 39, S=2)]
    for kw in cases:
        rc, text = call(**kw)
        assert rc != 0 and text.startswith("snvrag_typed_overlay: ") and len(text) > 30, (kw, rc, text)
    assert call(gt=None)[1] == "snvrag_typed_overlay: null pointer"
    assert "16-byte" in call(gt=gt + 4)[1] and "ld_bits" in call(ld=1)[1]
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == fill).all()), "a refused call wrote to a buffer it was passed"


def test_host_array_path_equals_the_device_path():
    c = make_case(5, 50, 5, 300, rows="random", extra_ld=2)
    c["site_row"][:12] = -1
    c["site_row"][12:] = np.random.default_rng(6).integers(0, 300, 38)
    c["site_row"][[20, 31]] = [300, -1]                                          # 36 typed rows among 50
    typed = int(((c["site_row"] >= 0) & (c["site_row"] < 300)).sum())
    rows_per_chunk = 7
    assert typed >= 3 * rows_per_chunk and typed % rows_per_chunk != 0           # >= 3 chunks, the last one short
    target = (c["alt"], c["miss"], 300, 5)
    spec = [nan_fill((50, 5)), nan_fill((50, 5)), nan_fill((50, 5, 4))]
    host = [a.copy() for a in spec]
    dev = [torch.from_numpy(a).to(DEV) for a in spec]
    m_spec = T.typed_overlay_host(*spec, c["alt"], c["miss"], 300, c["site_row"], c["col"])
    calls = []
    real = K.typed_overlay
    K.typed_overlay = lambda *a, **kw: (calls.append(a[0].shape[0]), real(*a, **kw))[1]
    try:
        m_host = T.typed_overlay(*host, target, c["site_row"], chunk_bytes=rows_per_chunk * 24 * 5 + 11)
        assert calls == [rows_per_chunk] * (typed // rows_per_chunk) + [typed % rows_per_chunk]
        m_dev = T.typed_overlay(*dev, tuple(torch.from_numpy(b).to(DEV) for b in target[:2]) + target[2:],
                                c["site_row"], c["col"])
    finally:
        K.typed_overlay = real
    assert m_host.dtype == m_dev.dtype == np.int32 and np.array_equal(m_host, m_spec) and np.array_equal(m_dev, m_spec)
    assert m_spec.sum() > 0
    for s, h, d in zip(spec, host, dev):
        assert same_bits(h, s) and same_bits(d.cpu().numpy(), s)


# --------------------------------------------------------------------------------------------- the entry point --
N_SITES, S_E2E = 1320, 3
ARGS = ["--synthetic", str(S_E2E), "--synthetic_sites", str(N_SITES), "--synthetic_ref", "24", "-d", "64", "-l", "1",
        "-a", "2", "-b", "4", "--k_retrieve", "3", "--mask_rate", "0.5", "--window_len", "1020",
        "--index_window_len", "1020"]


def records(text):
    return [ln for ln in text.split("\n") if ln and not ln.startswith("#")]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from src import infer_embedding_rag as I
    from src.dataset.synthetic import make_infer_arrays
    d = tmp_path_factory.mktemp("typed")
    out = dict(dir=d, arrays=make_infer_arrays(N_SITES, S_E2E, 24, missing_rate=0.5, seed=11))
    cases = dict(default=[], all_host=["--vcf_sites", "all"], all_device=["--vcf_sites", "all", "--vcf_writer", "device"],
                 all_host_df=["--vcf_sites", "all", "--device_features"],
                 all_device_df=["--vcf_sites", "all", "--device_features", "--vcf_writer", "device"])
    for name, extra in cases.items():
        I.infer(ARGS + extra + ["-o", str(d / name)])
        out[name] = (d / name / "imputed.vcf").read_text()
    return out


def test_all_sites_files_are_identical(runs):
    assert runs["all_host"] == runs["all_device"] == runs["all_host_df"] == runs["all_device_df"]
    assert runs["all_host"] != runs["default"]
    assert "ID=TYPED" not in runs["all_host"]                # INFO stays '.': nothing to declare
    h = lambda t: [ln for ln in t.split("\n") if ln.startswith("#")]
    assert h(runs["all_host"]) == h(runs["default"])


def test_all_sites_records(runs):
    a = runs["arrays"]
    ori_pos, rec, base = a["ori_pos"], records(runs["all_host"]), records(runs["default"])
    assert len(rec) == len(ori_pos) == N_SITES
    assert [int(r.split("\t")[1]) for r in rec] == ori_pos.tolist()
    z = np.load(runs["dir"] / "all_host" / "imputed.npz")
    z0 = np.load(runs["dir"] / "default" / "imputed.npz")
    flag = z["mask"][:, 0].astype(bool)
    assert set(z.files) == set(z0.files) | {"typed", "typed_missing"}
    assert z["typed"].dtype == np.bool_ and np.array_equal(z["typed"], ~flag) and 300 < flag.sum() < N_SITES - 300
    assert z["typed_missing"].dtype == np.int32 and z["typed_missing"].shape == (N_SITES,) and not z["typed_missing"].any()
    assert flag[1020:].any() and (~flag[1020:]).any()         # both kinds in the ragged second window
    # the imputed sites: the default run's records, byte for byte
    assert [r for r, f in zip(rec, flag) if f] == base and len(base) == int(flag.sum())
    # the typed sites: the target's genotypes, one-hot
    row = {int(p): i for i, p in enumerate(a["pos"])}
    for r, f, p in zip(rec, flag, ori_pos.tolist()):
        if not f:
            want = [CELL[tuple(a["vcf"][row[p], s].tolist())] for s in range(S_E2E)]
            assert r == f"21\t{p}\t.\t.\t.\t0.0\tPASS\t.\tGT:HDS:GP:DS\t" + "\t".join(want)
    # the arrays of the npz are the overlaid ones; the imputed rows are the default run's
    t = np.flatnonzero(~flag)
    assert np.array_equal(z["hap1"][t], a["vcf"][:, :, 0].astype(np.float32))
    assert np.array_equal(z["hap2"][t], a["vcf"][:, :, 1].astype(np.float32))
    assert np.array_equal(z["gp"][t].argmax(-1), 2 * a["vcf"][:, :, 0] + a["vcf"][:, :, 1])
    for k in ("hap1", "hap2", "gp"):
        assert np.array_equal(z[k][flag], z0[k][flag]) and not np.array_equal(z[k][t], z0[k][t])
    for name in ("all_device", "all_host_df", "all_device_df"):
        zz = np.load(runs["dir"] / name / "imputed.npz")
        for k in z.files:
            assert np.array_equal(z[k], zz[k]), (name, k)


def test_all_sites_with_info_bgzf_and_index(runs, capsys):
    from src import infer_embedding_rag as I
    a, d = runs["arrays"], runs["dir"]
    I.infer(ARGS + ["--vcf_sites", "all", "--vcf_info", "--vcf_bgzf", "--vcf_index", "--vcf_writer", "device",
                    "-o", str(d / "flags")])
    assert f"{len(a['pos'])} typed sites of {N_SITES}" in capsys.readouterr().out
    path = d / "flags" / "imputed.vcf.gz"
    text = gzip.decompress(path.read_bytes()).decode()
    assert text.count('##INFO=<ID=TYPED,Number=0,Type=Flag,Description="Site genotyped in the target">\n') == 1
    rec, plain = records(text), records(runs["all_host"])
    flag = np.load(d / "flags" / "imputed.npz")["mask"][:, 0].astype(bool)
    assert len(rec) == N_SITES
    for r, p, f in zip(rec, plain, flag):
        got, want = r.split("\t"), p.split("\t")
        assert got[:7] == want[:7] and got[8:] == want[8:]
        info = got[7].split(";")
        assert [x.split("=")[0] for x in info[:3]] == ["AF", "DR2", "R2"] and info[3:] == (["IMP"] if f else ["TYPED"])
    # a typed row: AF is the observed frequency, R2 = DR2 = 1 unless the site is monomorphic (then 0)
    row = {int(p): i for i, p in enumerate(a["pos"])}
    for r, f, p in zip(rec, flag, a["ori_pos"].tolist()):
        if not f:
            g = a["vcf"][row[p]]
            af = g.sum() / (2 * S_E2E)
            one = "0.000" if af in (0.0, 1.0) else "1.000"
            dr2 = "0.000" if len(set(g.sum(1).tolist())) == 1 else "1.000"
            assert r.split("\t")[7] == f"AF={af:.4f};DR2={dr2};R2={one};TYPED"
    # a region through the written index: typed and imputed records of the span
    lo, hi = 400, 460
    span = a["ori_pos"][lo:hi + 1]
    assert flag[lo:hi + 1].any() and (~flag[lo:hi + 1]).any()
    got = V.read_vcf(path, DEV, region=("21", int(span[0]), int(span[-1])))
    assert np.array_equal(got.pos, span)
    gt = got.gt()
    for i in np.flatnonzero(~flag[lo:hi + 1]):
        assert np.array_equal(gt[i], a["vcf"][row[int(span[i])]])


# ------------------------------------------------------------------------------- a VCF target with '.' calls --
def write_panel_file(path, names, pops):
    with open(path, "w") as f:
        f.write("sample\tpop\tsuper_pop\tgender\n")
        for s, p in zip(names, pops):
            f.write(f"{s}\tX\t{p}\tmale\n")


def test_vcf_target_with_missing_calls(tmp_path, capsys):
    """A target read from a VCF (the device bit rows of the reader, pitch ceil(n / 8)) with three '.' calls: they
    are counted in ``typed_missing`` and keep the model's values; every other typed cell is the observed call."""
    from src import infer_embedding_rag as I
    from src.dataset.synthetic import POPS, make_infer_arrays
    a = make_infer_arrays(1300, 4, 24, missing_rate=0.3, seed=11)
    vcf = a["vcf"].copy()
    vcf[5, 1, 0] = -1                                        # half missing
    vcf[9, 2] = -1
    vcf[len(vcf) - 1, 0, 1] = -1                             # the last record
    samples, refs = [f"S{i}" for i in range(4)], [f"R{i}" for i in range(24)]
    V.write_gt_vcf(tmp_path / "target.vcf", samples, a["pos"], vcf, chrom="21")
    V.write_gt_vcf(tmp_path / "panel.vcf.gz", refs, a["ref_pos"], a["ref_gt"], chrom="21")
    write_panel_file(tmp_path / "target.panel", samples, a["pops"])
    write_panel_file(tmp_path / "panel.panel", refs, [POPS[(3 * i) % 5] for i in range(24)])
    common = ["--infer_dataset", str(tmp_path / "target.vcf"), "--infer_panel", str(tmp_path / "target.panel"),
              "--ref_panel", str(tmp_path / "panel.vcf.gz"), "--ref_panel_pops", str(tmp_path / "panel.panel"),
              "-d", "64", "-l", "1", "-a", "2", "-b", "4", "--k_retrieve", "3", "--index_window_len", "1020"]
    I.infer(common + ["--no_vcf", "-o", str(tmp_path / "default")])
    capsys.readouterr()
    I.infer(common + ["--vcf_sites", "all", "-o", str(tmp_path / "all")])
    assert "3 cells keep the model's output" in capsys.readouterr().out
    z, z0 = np.load(tmp_path / "all" / "imputed.npz"), np.load(tmp_path / "default" / "imputed.npz")
    site = np.searchsorted(a["ori_pos"], a["pos"])           # the site row of every target record
    want = np.zeros(1300, np.int32)
    want[site[[5, 9, len(vcf) - 1]]] = 1
    assert np.array_equal(z["typed_missing"], want) and np.array_equal(z["typed"], np.isin(a["ori_pos"], a["pos"]))
    called = (vcf >= 0).all(-1)                              # [records, samples]
    for k, obs in (("hap1", vcf[:, :, 0]), ("hap2", vcf[:, :, 1])):
        assert np.array_equal(z[k][site][called], obs[called].astype(np.float32))
        assert np.array_equal(z[k][site][~called], z0[k][site][~called])      # the model's values
        assert np.array_equal(z[k][~z["typed"]], z0[k][~z["typed"]])
    assert np.array_equal(z["gp"][site][~called], z0["gp"][site][~called])
    rec = records((tmp_path / "all" / "imputed.vcf").read_text())
    assert len(rec) == 1300
    cells = rec[site[9]].split("\t")[9:]
    h = lambda s: "%.3f,%.3f" % (z0["hap1"][site[9], s], z0["hap2"][site[9], s])
    assert cells[2].split(":")[1] == h(2) and cells[2] not in CELL.values()
    assert cells[0] == CELL[tuple(vcf[9, 0].tolist())]
