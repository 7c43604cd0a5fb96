"""Per-site imputation quality on the GPU (csrc/quality.hip ``snvrag_site_stats``, src/quality.py, the writers'
``info=``, ``--vcf_info`` / ``--truth_vcf``).

The kernel against ``math.fsum`` sums of the specification's terms: one 64-lane wave per site, four sites per
workgroup, a lane's samples 64 apart and four of them in flight, so the sample counts straddle 64 (the wave),
128 and 256 (one round of a wave), and the site counts leave a workgroup partly empty.  Integer tables are
equal; a float sum of ``count`` exactly representable terms is within ``count * 2^-52 * sum|term|`` of the
exact sum (any order errs by at most (count - 1) 2^-53 sum|term| to first order: a factor 2 is left)."""
import functools
import gzip
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_vcf_writer import CHROM, N_SITES, case, device_bytes, first_difference, host_bytes
from test_vcf_writer_cpu import boundary_values

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
N_MAX = 37
S_LIST = [1, 2, 3, 63, 64, 65, 127, 129, 255, 256, 257, 700]
EPS = 2.0 ** -52


def _fsum_rows(a):
    return np.asarray([math.fsum(r) for r in np.asarray(a, np.float64).tolist()], np.float64)


@functools.lru_cache(maxsize=None)
def inputs(S):
    """37 sites x S samples with a truth of 41 records x S + 3 columns (read-only), and the reference: the
    float sums by math.fsum over the exact float64 terms, with sum|term| and the number of terms of each."""
    from src.quality import called_alt_count
    rng = np.random.default_rng(1000 + S)
    n = N_MAX
    pool = boundary_values()
    small = pool[pool <= np.nextafter(np.float32(2), np.float32(3))]
    gt = rng.dirichlet(np.ones(4), (n, S)).astype(np.float32)              # ordinary probabilities
    h1, h2 = rng.random((n, S), dtype=np.float32), rng.random((n, S), dtype=np.float32)
    for r in range(1, n, 3):                                               # the writer tests' boundary values
        gt[r], h1[r], h2[r] = rng.choice(small, (S, 4)), rng.choice(small, S), rng.choice(small, S)
    gt[6] = np.float32(0.25)                                               # exact ties: the first wins
    gt[9] = np.float32([0, 0.5, 0.5, 0])
    h1[12], h2[12], gt[12] = 0, 0, 0                                       # a site no window covered
    n_truth, S_truth = n + 4, S + 3
    truth = rng.integers(0, 2, (n_truth, S_truth, 2)).astype(np.int8)
    truth[rng.random((n_truth, S_truth)) < 0.05] = -1                      # missing calls
    truth[:, 0, 1] = -1                                                    # one sample missing one haplotype
    truth_col = rng.permutation(S_truth)[:S].astype(np.int32)
    truth_row = rng.permutation(n_truth)[:n].astype(np.int32)
    truth_col[rng.random(S) < 0.1] = -1
    truth_row[rng.random(n) < 0.1] = -1
    truth_row[4] = -1
    if truth_row[0] < 0:
        truth_row[0] = 1                                                   # n = 1 keeps a truth row
    if S >= 3:
        truth_col[1] = -1
        if not (truth_col == 0).any():
            truth_col[2] = 0                                               # the half-missing sample is read
    for a in (h1, h2, gt, truth, truth_row, truth_col):
        a.setflags(write=False)

    gp1 = gt[..., 1] + gt[..., 2]
    ds = gp1 + np.float32(2) * gt[..., 3]
    e = ds.astype(np.float64)
    f = gp1.astype(np.float64) + 4.0 * gt[..., 3].astype(np.float64)
    d1, d2 = h1.astype(np.float64), h2.astype(np.float64)
    tv = truth[np.maximum(truth_row, 0)][:, np.maximum(truth_col, 0)]
    ok = (truth_row >= 0)[:, None] & (truth_col >= 0)[None, :] & (tv[..., 0] >= 0) & (tv[..., 1] >= 0)
    t = tv.astype(np.int64).sum(-1)
    cell = 3 * t + called_alt_count(gt)
    table = np.stack([(ok & (cell == k)).sum(1) for k in range(9)], 1).astype(np.int32)
    ez = np.where(ok, e, 0.0)
    est_terms = [np.concatenate([d1, d2], 1), np.concatenate([d1 * d1, d2 * d2], 1), e, e * e, f]
    acc_terms = [ez, ez * ez, ez * t]
    est = np.stack([_fsum_rows(x) for x in est_terms], 1)
    acc = np.stack([_fsum_rows(x) for x in acc_terms], 1)
    est_bound = np.stack([x.shape[1] * EPS * _fsum_rows(np.abs(x)) for x in est_terms], 1)
    acc_bound = np.stack([ok.sum(1) * EPS * _fsum_rows(np.abs(x)) for x in acc_terms], 1)
    return dict(h1=h1, h2=h2, gt=gt, truth=truth, truth_row=truth_row, truth_col=truth_col, est=est, acc=acc,
                table=table, est_bound=est_bound, acc_bound=acc_bound)


def dev_args(c, n):
    t = lambda a: torch.from_numpy(np.array(a)).to(DEV)            # a writable copy of the read-only input
    return (t(c["h1"][:n]), t(c["h2"][:n]), t(c["gt"][:n])), (t(c["truth"]), t(c["truth_row"][:n]), t(c["truth_col"]))


@pytest.mark.parametrize("n", [1, 5, 37])
@pytest.mark.parametrize("S", S_LIST)
def test_kernel_matches_the_specification(S, n):
    from src import kernels as K
    c = inputs(S)
    arrays, truth = dev_args(c, n)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    est, acc, table = K.site_stats(*arrays, *truth, bad)
    est2, acc2, table2 = K.site_stats(*arrays, *truth, bad)
    only, none_acc, none_table = K.site_stats(*arrays)
    assert int(bad.item()) == 0 and none_acc is None and none_table is None
    assert est.dtype == acc.dtype == torch.float64 and table.dtype == torch.int32
    assert est.shape == (n, 5) and acc.shape == (n, 3) and table.shape == (n, 9)
    # two launches, and the launch without truth, give the same bits
    assert torch.equal(est.view(torch.int64), est2.view(torch.int64)) and torch.equal(table, table2)
    assert torch.equal(acc.view(torch.int64), acc2.view(torch.int64))
    assert torch.equal(est.view(torch.int64), only.view(torch.int64))
    est, acc, table = est.cpu().numpy(), acc.cpu().numpy(), table.cpu().numpy()
    assert np.array_equal(table, c["table"][:n])
    err_e, err_a = np.abs(est - c["est"][:n]), np.abs(acc - c["acc"][:n])
    print("max error / bound: est", float(np.max(err_e / np.maximum(c["est_bound"][:n], 1e-300))),
          "acc", float(np.max(err_a / np.maximum(c["acc_bound"][:n], 1e-300))))
    assert (err_e <= c["est_bound"][:n]).all(), (err_e - c["est_bound"][:n]).max()
    assert (err_a <= c["acc_bound"][:n]).all(), (err_a - c["acc_bound"][:n]).max()
    # what the inputs set out to cover
    assert c["table"][4].sum() == 0 and c["truth_row"][0] >= 0
    if S >= 3:
        assert (c["truth_col"] == -1).any() and (c["truth_row"] == -1).any() and (c["truth_col"] == 0).any()
    if S >= 63:
        assert c["table"][0].sum() > S // 2 and (c["table"].sum(0) > 0).all()      # every cell of the 3 x 3 table is hit


def test_specification_in_numpy_agrees_with_the_reference():
    """``site_stats_host`` (what the end-to-end test scores against) on the same inputs, the same bound."""
    from src.quality import site_stats_host
    c = inputs(257)
    est, acc, table = site_stats_host(c["h1"], c["h2"], c["gt"], c["truth"], c["truth_row"], c["truth_col"])
    assert np.array_equal(table, c["table"])
    assert (np.abs(est - c["est"]) <= c["est_bound"]).all() and (np.abs(acc - c["acc"]) <= c["acc_bound"]).all()


def test_indices_out_of_range_are_counted_and_read_nothing():
    from src import kernels as K
    c = inputs(65)
    n, S = N_MAX, 65
    n_truth, S_truth = c["truth"].shape[:2]
    arrays, (truth, row, col) = dev_args(c, n)
    keep = [i for i in range(n) if i not in (2, 3)]
    row_bad, col_bad, row_m1, col_m1 = row.clone(), col.clone(), row.clone(), col.clone()
    row_bad[2], row_bad[3], row_m1[2], row_m1[3] = n_truth, -5, -1, -1
    col_bad[7], col_bad[64], col_m1[7], col_m1[64] = S_truth, -(1 << 31), -1, -1
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    est, acc, table = K.site_stats(*arrays, truth, row_bad, col_bad, bad)
    assert int(bad.item()) == 4                                  # two rows, two columns: each once
    bad.zero_()
    est1, acc1, table1 = K.site_stats(*arrays, truth, row_m1, col_m1, bad)
    assert int(bad.item()) == 0
    assert torch.equal(table, table1) and torch.equal(acc.view(torch.int64), acc1.view(torch.int64))
    assert torch.equal(est.view(torch.int64), est1.view(torch.int64))
    assert int(table[2].sum()) == 0 and int(table[3].sum()) == 0 and float(acc[2:4].abs().sum()) == 0
    # the other sites: what the good indices give, but for the two samples whose columns went away
    _, acc0, table0 = K.site_stats(*arrays, truth, row, col_m1, bad)
    assert torch.equal(table[keep], table0[keep]) and torch.equal(acc[keep].view(torch.int64), acc0[keep].view(torch.int64))
    # the high-level call refuses them
    from src.quality import site_stats
    with pytest.raises(ValueError, match="outside the truth array"):
        site_stats(*arrays, truth, row_bad, col)


def test_entry_point_refuses_bad_arguments():
    from src import native as N
    from src.native import check, ptr, stream_ptr
    c = inputs(3)
    (h1, h2, gt), (truth, row, col) = dev_args(c, 5)
    est = torch.empty(5, 5, dtype=torch.float64, device=DEV)
    acc = torch.empty(5, 3, dtype=torch.float64, device=DEV)
    table = torch.empty(5, 9, dtype=torch.int32, device=DEV)
    bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_truth, S_truth = truth.shape[:2]
    good = dict(n=5, S=3, h1=ptr(h1), h2=ptr(h2), gt=ptr(gt), truth=ptr(truth), n_truth=n_truth, S_truth=S_truth,
                row=ptr(row), col=ptr(col), est=ptr(est), acc=ptr(acc), table=ptr(table), bad=ptr(bad))

    def call(**kw):
        a = {**good, **kw}
        check(N.lib().snvrag_site_stats(a["n"], a["S"], a["h1"], a["h2"], a["gt"], a["truth"], a["n_truth"],
                                        a["S_truth"], a["row"], a["col"], a["est"], a["acc"], a["table"], a["bad"],
                                        stream_ptr()), "site_stats")

    call()
    call(truth=None, row=None, col=None, acc=None, table=None, bad=None)        # est only: none of them needed
    for kw, msg in ((dict(h1=None), "null"), (dict(h2=None), "null"), (dict(gt=None), "null"), (dict(est=None), "null"),
                    (dict(n=0), "n must"), (dict(S=0), "S must"), (dict(S=1 << 31), "S must"),
                    (dict(gt=ptr(gt) + 4), "aligned"), (dict(row=None), "truth needs"), (dict(col=None), "truth needs"),
                    (dict(acc=None), "truth needs"), (dict(table=None), "truth needs"), (dict(bad=None), "truth needs"),
                    (dict(n_truth=0), "n_truth")):
        with pytest.raises(RuntimeError, match=msg):
            call(**kw)
    torch.cuda.synchronize()


def test_chunked_upload_gives_the_device_tensor_result():
    from src.quality import CELL_BYTES, site_stats
    S = 129
    c = inputs(S)
    arrays, truth = dev_args(c, N_MAX)
    want = site_stats(*arrays, *truth)
    chunk = CELL_BYTES * S * 5 + 7                              # 5 rows a chunk: 37 = 7 * 5 + 2
    got = site_stats(c["h1"], c["h2"], c["gt"], c["truth"], c["truth_row"], c["truth_col"], device=DEV, chunk_bytes=chunk)
    one = site_stats(c["h1"], c["h2"], torch.from_numpy(c["gt"].copy()), device=DEV, chunk_bytes=1)     # a row a chunk
    bits = lambda x: x.view(np.int64) if x.dtype == np.float64 else x
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(bits(g), bits(w))
    assert np.array_equal(bits(one[0]), bits(want[0])) and one[1] is None and one[2] is None
    assert np.array_equal(want[2], c["table"])


def _info(c):
    from src.quality import estimates, info_strings, site_stats_host
    est, _, _ = site_stats_host(c["h1"], c["h2"], c["gt"])
    return info_strings(*estimates(est, c["h1"].shape[1]))


@pytest.mark.parametrize("S", [1, 257])
def test_device_writer_info_equals_host_writer_bytes(tmp_path, S):
    c = case(S)
    info = _info(c)
    assert len(set(info)) > 3 and len(set(map(len, info))) == 1
    info = [s if i % 5 else s.replace(";IMP", ";IMP;X=" + "y" * (i % 16)) for i, s in enumerate(info)]   # any width
    flag = np.random.default_rng(8).random(N_SITES) < 0.7
    want = host_bytes(tmp_path, c, info=info, pos_flag=flag)
    plain = host_bytes(tmp_path, c, name="plain.vcf", pos_flag=flag)
    assert want.count(b"\n") == plain.count(b"\n") + 4 and want.count(b"##INFO=<ID=") == 4
    assert want.count(b";IMP") == int(flag.sum()) and plain.count(b";IMP") == 0
    for form in ("device", "numpy"):
        assert first_difference(device_bytes(tmp_path, c, form=form, info=info, pos_flag=flag), want) is None
    # info=None: today's bytes from both writers
    assert first_difference(device_bytes(tmp_path, c, info=None, pos_flag=flag), plain) is None
    # bgzipped: inflates to the same text
    z = device_bytes(tmp_path, c, name="dev.vcf.gz", info=info, pos_flag=flag, bgzf=True)
    assert z[:4] == b"\x1f\x8b\x08\x04" and first_difference(gzip.decompress(z), want) is None
    zh = host_bytes(tmp_path, c, name="host.vcf.gz", info=info, pos_flag=flag, bgzf=True)
    assert first_difference(gzip.decompress(zh), want) is None


@pytest.mark.parametrize("bgzf", [False, True])
def test_device_writer_info_survives_the_bad_value_fallback(tmp_path, capsys, bgzf):
    base = case(257)
    c = dict(base, h1=base["h1"].copy())
    c["h1"][11, 200] = np.nan
    info = _info(base)
    want = host_bytes(tmp_path, c, info=info)
    out = tmp_path / "out"
    out.mkdir()
    got = device_bytes(out, c, expect=False, info=info, bgzf=bgzf)
    assert first_difference(gzip.decompress(got) if bgzf else got, want) is None
    assert os.listdir(out) == ["dev.vcf"] and "host writer" in capsys.readouterr().out


def _records(text):
    """(pos, {AF, DR2, R2} as printed) of every body line, and the header lines."""
    body, header = [], []
    for line in text.split("\n"):
        if line.startswith("#"):
            header.append(line)
        elif line:
            col = line.split("\t", 9)
            kv = dict(f.split("=") for f in col[7].split(";") if "=" in f)
            assert col[7].endswith(";IMP") and list(kv) == ["AF", "DR2", "R2"]
            assert [len(kv[k].split(".")[1]) for k in ("AF", "DR2", "R2")] == [4, 3, 3]
            body.append((int(col[1]), {k: float(v) for k, v in kv.items()}))
    return body, header


def test_infer_cli_writes_info_and_scores_against_the_truth(tmp_path, capsys):
    """``--vcf_info --truth_vcf`` through the entry point with the host writer, then with the device writer
    from the scatter path's device arrays (bgzipped; the truth file bgzipped and inflated on the device too):
    one VCF text, INFO as the specification gives it on imputed.npz, accuracy.tsv as ``aggregate`` of the
    specification; and a run without the new flags writes the two files it always wrote."""
    from src import infer_embedding_rag as I
    from src import quality as Q
    from src.dataset.synthetic import make_infer_arrays
    from src.dataset.vcf_reader import write_gt_vcf
    n_sites, S = 2040, 6
    a = make_infer_arrays(n_sites, S, 24, missing_rate=0.5, seed=11)
    names = [f"S{i}" for i in range(S)]
    write_gt_vcf(tmp_path / "truth.vcf", names, a["ori_pos"], a["truth"], chrom="21")
    write_gt_vcf(tmp_path / "truth.vcf.gz", names, a["ori_pos"], a["truth"], chrom="21", bgzf=True)
    args = ["--synthetic", str(S), "--synthetic_sites", str(n_sites), "--synthetic_ref", "24", "-d", "64", "-l", "2",
            "-a", "2", "-b", "4", "--k_retrieve", "3", "--mask_rate", "0.5", "--index_window_len", "1020"]
    I.infer(args + ["-o", str(tmp_path / "plain")])
    assert sorted(os.listdir(tmp_path / "plain")) == ["imputed.npz", "imputed.vcf"]
    new = ["--vcf_info", "--truth_vcf"]
    I.infer(args + new + [str(tmp_path / "truth.vcf"), "--vcf_writer", "host", "-o", str(tmp_path / "host")])
    capsys.readouterr()
    I.infer(args + new + [str(tmp_path / "truth.vcf.gz"), "--vcf_inflate", "device", "--vcf_writer", "device",
                          "--device_features", "--vcf_bgzf", "-o", str(tmp_path / "device")])
    printed = capsys.readouterr().out
    from src.dataset.vcf_reader import set_default_inflate
    set_default_inflate("host")                                  # the entry point's --vcf_inflate is process-wide
    assert sorted(os.listdir(tmp_path / "host")) == ["accuracy.tsv", "imputed.npz", "imputed.vcf", "quality.npz"]
    assert sorted(os.listdir(tmp_path / "device")) == ["accuracy.tsv", "imputed.npz", "imputed.vcf.gz", "quality.npz"]
    text = (tmp_path / "host" / "imputed.vcf").read_text()
    assert gzip.decompress((tmp_path / "device" / "imputed.vcf.gz").read_bytes()).decode() == text
    plain = (tmp_path / "plain" / "imputed.vcf").read_text()
    from src.vcf_device import INFO_HEADER
    assert INFO_HEADER in text and text.replace(INFO_HEADER, "").count("\n") == plain.count("\n")

    z = np.load(tmp_path / "host" / "imputed.npz")
    h1, h2, gt, flag = z["hap1"], z["hap2"], z["gp"], z["mask"][:, 0].astype(bool)
    truth_row = np.where(flag, np.arange(n_sites), -1)
    est, acc, table = Q.site_stats_host(h1, h2, gt, a["truth"], truth_row, np.arange(S))
    af, r2, dr2 = Q.estimates(est, S)
    body, header = _records(text)
    assert [p for p, _ in body] == a["ori_pos"][flag].tolist() and 500 < len(body) < 1500
    assert sum(l.startswith("##INFO=<ID=") for l in header) == 4
    # the kernel's sums and the specification's differ by the summation order: at most 2 S 2^-52 sum|term|, a relative
    # 3e-15 here, which the ratios enlarge by the inverse of their denominators (checked below to exceed 1e-4 where
    # they are not exactly 0): 1e-9 covers it, beside half a unit of the last printed digit
    den_r2, den_dr2 = af * (1 - af), est[:, 4] - est[:, 2] ** 2 / S
    for den in (den_r2[flag], den_dr2[flag]):
        assert ((den == 0) | (den > 1e-4)).all()
    for (p, kv), i in zip(body, np.flatnonzero(flag)):
        assert abs(kv["AF"] - af[i]) <= 0.5e-4 + 1e-9, (p, kv, af[i])
        assert abs(kv["DR2"] - dr2[i]) <= 0.5e-3 + 1e-9, (p, kv, dr2[i])
        assert abs(kv["R2"] - r2[i]) <= 0.5e-3 + 1e-9, (p, kv, r2[i])
    print("distinct printed values:", {k: len({kv[k] for _, kv in body}) for k in ("AF", "DR2", "R2")})

    gaf = a["freq"][3][5].astype(np.float64)
    want = Q.aggregate(acc[flag], table[flag], np.minimum(gaf, 1 - gaf)[flag])
    tsv = (tmp_path / "host" / "accuracy.tsv").read_text()
    assert (tmp_path / "device" / "accuracy.tsv").read_text() == tsv
    lines = tsv.rstrip("\n").split("\n")
    assert lines[0].split("\t") == list(Q.TSV_COLUMNS) and len(lines) == len(want) + 1 == 9
    for line, w in zip(lines[1:], want):
        col = line.split("\t")
        assert col[0] == w["maf_bin"] and int(col[1]) == w["sites"] and int(col[2]) == w["genotypes"]
        for v, k in zip(col[3:], Q.TSV_COLUMNS[3:]):
            assert len(v.split(".")[-1]) == 6 or v == "nan"
            assert (v == "nan") == math.isnan(w[k]) and (v == "nan" or abs(float(v) - w[k]) <= 0.5e-6 + 1e-9), (line, w)
    assert want[-1]["sites"] == int(flag.sum()) and want[-1]["genotypes"] == S * int(flag.sum())
    assert sum(w["sites"] for w in want[:-1]) == want[-1]["sites"] and sum(w["sites"] > 0 for w in want[:-1]) >= 3
    assert lines[-1].replace("\t", " ") in printed               # the ALL row is printed
    q = np.load(tmp_path / "device" / "quality.npz")
    qh = np.load(tmp_path / "host" / "quality.npz")
    assert q.files == qh.files and all(np.array_equal(q[k], qh[k], equal_nan=True) for k in q.files)
    assert np.array_equal(q["table"], table) and np.array_equal(q["pos"], a["ori_pos"]) and np.array_equal(q["flag"], flag)
    assert np.array_equal(q["truth_row"], truth_row)
