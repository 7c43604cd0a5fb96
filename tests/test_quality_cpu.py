"""Per-site imputation quality without a GPU (src/quality.py): the numpy specification ``site_stats_host``
against explicit Python loops summed with ``math.fsum``, the figures derived from the sums (``estimates``,
``accuracy``, ``aggregate``), the site / sample maps, the INFO strings and the host writer's ``info=``."""
import math
import types

import numpy as np
import pytest


def loop_stats(h1, h2, gt, truth=None, truth_row=None, truth_col=None):
    """The definitions, one sample at a time; every sum by math.fsum (exact, rounded once).  Also returns the
    sum of the absolute terms of every float sum (what an error bound of a summation scales with)."""
    n, S = h1.shape
    est, mag = np.zeros((n, 5)), np.zeros((n, 8))
    acc, table = np.zeros((n, 3)), np.zeros((n, 9), np.int32)
    for i in range(n):
        terms = [[] for _ in range(8)]
        r = -1 if truth is None else int(truth_row[i])
        r = r if truth is not None and 0 <= r < truth.shape[0] else -1
        for s in range(S):
            g = gt[i, s]
            gp1 = np.float32(g[1] + g[2])
            ds = np.float32(gp1 + np.float32(np.float32(2) * g[3]))
            e = float(ds)
            f = float(gp1) + 4.0 * float(g[3])
            a, b = float(h1[i, s]), float(h2[i, s])
            terms[0] += [a, b]
            terms[1] += [a * a, b * b]
            terms[2].append(e)
            terms[3].append(e * e)
            terms[4].append(f)
            if r < 0:
                continue
            c = int(truth_col[s])
            if not 0 <= c < truth.shape[1]:
                continue
            t0, t1 = int(truth[r, c, 0]), int(truth[r, c, 1])
            if t0 < 0 or t1 < 0:
                continue
            t = t0 + t1
            k = 0
            for j in (1, 2, 3):                       # the first maximum
                if g[j] > g[k]:
                    k = j
            table[i, 3 * t + (0, 1, 1, 2)[k]] += 1
            terms[5].append(e)
            terms[6].append(e * e)
            terms[7].append(e * t)
        for q in range(8):
            (est if q < 5 else acc)[i, q if q < 5 else q - 5] = math.fsum(terms[q])
            mag[i, q] = math.fsum(abs(v) for v in terms[q])
    return est, acc, table, mag


def small_case():
    """7 sites x 5 samples; truth 9 records x 6 columns, permuted both ways."""
    rng = np.random.default_rng(7)
    n, S = 7, 5
    gt = rng.dirichlet(np.ones(4), (n, S)).astype(np.float32)
    h1, h2 = rng.random((n, S), dtype=np.float32), rng.random((n, S), dtype=np.float32)
    gt[1] = np.float32(0.25)                                   # an exact tie: index 0 wins
    gt[2, :, :] = np.float32([0, 0.5, 0.5, 0])                 # a tie of 1 and 2: index 1 wins (one ALT either way)
    gt[2, 0] = np.float32([0.1, 0.2, 0.35, 0.35])              # a tie of 2 and 3: index 2 wins (one ALT, not two)
    h1[4], h2[4], gt[4] = 0, 0, 0                              # a site no window covered
    truth = rng.integers(0, 2, (9, 6, 2)).astype(np.int8)
    truth[3, 2] = (-1, -1)                                     # a missing call
    truth[3, 4] = (1, -1)                                      # one haplotype missing
    truth[8, 0] = (-1, 0)
    truth_row = np.asarray([3, 8, 0, -1, 5, 1, 7], np.int32)   # permuted; site 3 is not in the truth file
    truth_col = np.asarray([4, 2, -1, 0, 5], np.int32)         # permuted; sample 2 is not in the truth file
    return h1, h2, gt, truth, truth_row, truth_col


def test_site_stats_host_matches_explicit_loops():
    from src.quality import site_stats_host
    h1, h2, gt, truth, row, col = small_case()
    want_est, want_acc, want_table, mag = loop_stats(h1, h2, gt, truth, row, col)
    for block_rows in (64, 3):
        est, acc, table = site_stats_host(h1, h2, gt, truth, row, col, block_rows=block_rows)
        assert est.dtype == acc.dtype == np.float64 and table.dtype == np.int32
        assert np.array_equal(table, want_table)
        # 10 terms at most: any-order float64 summation of exact terms is within count 2^-52 sum|term|
        assert (np.abs(est - want_est) <= 10 * 2.0 ** -52 * mag[:, :5]).all()
        assert (np.abs(acc - want_acc) <= 10 * 2.0 ** -52 * mag[:, 5:]).all()
    assert want_table[3].sum() == 0 and (want_acc[3] == 0).all()          # no truth row: zeros
    assert want_table[0].sum() == 2                                        # 4 columns, two with a missing allele
    assert want_table[1].sum() == 3 and (want_table[1].reshape(3, 3)[:, 1:] == 0).all()      # the tie calls 0|0
    assert (want_table[2].reshape(3, 3)[:, 1].sum() == 4)                  # both ties call one ALT
    assert (est[4] == 0).all() and table[4].sum() == 4 and (acc[4] == 0).all()
    only, none_acc, none_table = site_stats_host(h1, h2, gt)
    assert np.array_equal(only, est) and none_acc is None and none_table is None
    # an index outside the truth array behaves as -1
    row2, col2 = row.copy(), col.copy()
    row2[0], col2[1] = 9, 6
    _, acc2, table2 = site_stats_host(h1, h2, gt, truth, row2, col2)
    row3, col3 = row.copy(), col.copy()
    row3[0], col3[1] = -1, -1
    _, acc3, table3 = site_stats_host(h1, h2, gt, truth, row3, col3)
    assert np.array_equal(acc2, acc3) and np.array_equal(table2, table3) and table2[0].sum() == 0
    with pytest.raises(TypeError):
        site_stats_host(h1.astype(np.float64), h2, gt)


def test_estimates_on_certain_monomorphic_and_uncertain_sites():
    from src.quality import estimates, site_stats_host
    S = 8
    hap = np.zeros((3, S, 2), np.float32)
    hap[0, :2, 0] = 1
    hap[0, 0, 1] = 1                                            # 3 ALT of 16: af 0.1875
    hap[2] = 0.25                                               # every sample equally unsure
    gt = np.zeros((3, S, 4), np.float32)
    for i in range(3):
        a, b = hap[i, :, 0], hap[i, :, 1]
        gt[i] = np.stack([(1 - a) * (1 - b), (1 - a) * b, a * (1 - b), a * b], -1)
    est, _, _ = site_stats_host(hap[..., 0].copy(), hap[..., 1].copy(), gt)
    af, r2, dr2 = estimates(est, S)
    assert af.dtype == r2.dtype == dr2.dtype == np.float64
    assert af.tolist() == [3 / 16, 0.0, 0.25]
    assert r2[0] == pytest.approx(1.0, abs=1e-12) and dr2[0] == pytest.approx(1.0, abs=1e-12)
    assert r2[1] == 0.0 and dr2[1] == 0.0                       # monomorphic: both denominators are 0
    assert r2[2] == 0.0 and dr2[2] == 0.0                       # no variance between samples
    assert ((0 <= r2) & (r2 <= 1) & (0 <= dr2) & (dr2 <= 1)).all()


def test_accuracy_r2_is_the_squared_pearson_correlation():
    from src.quality import accuracy, site_stats_host
    rng = np.random.default_rng(3)
    n, S = 6, 40
    gt = rng.dirichlet(np.ones(4), (n, S)).astype(np.float32)
    h = rng.random((n, S), dtype=np.float32)
    truth = rng.integers(0, 2, (n, S, 2)).astype(np.int8)
    truth[4] = 1                                                # the truth does not vary
    gt[5] = np.float32([0.5, 0.25, 0.25, 0])                    # the dosage does not vary (0.5 everywhere)
    _, acc, table = site_stats_host(h, h, gt, truth, np.arange(n), np.arange(S))
    got = accuracy(acc, table)
    ds = ((gt[..., 1] + gt[..., 2]) + 2 * gt[..., 3]).astype(np.float64)
    t = truth.sum(-1).astype(np.float64)
    for i in range(4):
        assert got["r2"][i] == pytest.approx(np.corrcoef(ds[i], t[i])[0, 1] ** 2, abs=1e-12)
    assert np.isnan(got["r2"][4]) and np.isnan(got["r2"][5])
    assert got["n"].tolist() == [S] * n and got["n"].dtype == np.int64
    c = np.asarray([0, 1, 1, 2])[np.argmax(gt, -1)]
    for i in range(n):
        assert got["concordance"][i] == pytest.approx((c[i] == t[i]).mean(), abs=1e-15)
        nr = t[i] >= 1
        assert got["nonref_concordance"][i] == pytest.approx((c[i] == t[i])[nr].mean(), abs=1e-15)
    empty = accuracy(np.zeros((1, 3)), np.zeros((1, 9), np.int32))
    assert empty["n"][0] == 0 and all(np.isnan(empty[k][0]) for k in ("r2", "concordance", "nonref_concordance"))


def test_aggregate_bins_edges_and_pools():
    from src.quality import DEFAULT_MAF_EDGES, accuracy, aggregate, site_stats_host
    rng = np.random.default_rng(5)
    maf = np.asarray([0.0, 0.0005, 0.001, 0.005, 0.0099, 0.01, 0.05, 0.1, 0.2, 0.3, 0.5, 0.5])
    n, S = len(maf), 30
    gt = rng.dirichlet(np.ones(4), (n, S)).astype(np.float32)
    h = rng.random((n, S), dtype=np.float32)
    truth = rng.integers(0, 2, (n, S, 2)).astype(np.int8)
    truth[1] = 0                                                # r2 undefined at this site
    _, acc, table = site_stats_host(h, h, gt, truth, np.arange(n), np.arange(S))
    rows = aggregate(acc, table, maf)
    assert [r["maf_bin"] for r in rows] == ["[0,0.001)", "[0.001,0.005)", "[0.005,0.01)", "[0.01,0.05)", "[0.05,0.1)",
                                            "[0.1,0.2)", "[0.2,0.5]", "ALL"]
    assert len(DEFAULT_MAF_EDGES) == 8
    # 0.001 lands in the second bin, 0.5 in the last; ALL holds every site
    assert [r["sites"] for r in rows] == [2, 1, 2, 1, 1, 1, 4, n]
    assert [r["genotypes"] for r in rows] == [S * r["sites"] for r in rows]
    ds = ((gt[..., 1] + gt[..., 2]) + 2 * gt[..., 3]).astype(np.float64)
    t = truth.sum(-1).astype(np.float64)
    c = np.asarray([0, 1, 1, 2])[np.argmax(gt, -1)]
    site_r2 = accuracy(acc, table)["r2"]
    members = [[0, 1], [2], [3, 4], [5], [6], [7], [8, 9, 10, 11], list(range(n))]
    for r, m in zip(rows, members):
        e, tt, cc = ds[m].ravel(), t[m].ravel(), c[m].ravel()                 # the bin's genotypes, concatenated
        assert r["pooled_r2"] == pytest.approx(np.corrcoef(e, tt)[0, 1] ** 2, abs=1e-12)
        assert r["concordance"] == pytest.approx((cc == tt).mean(), abs=1e-15)
        assert r["nonref_concordance"] == pytest.approx((cc == tt)[tt >= 1].mean(), abs=1e-15)
        assert r["mean_r2"] == pytest.approx(np.nanmean(site_r2[m]), abs=1e-15)
    assert rows[0]["mean_r2"] == pytest.approx(site_r2[0], abs=1e-15)          # site 1 is left out of the mean
    custom = aggregate(acc, table, maf, (0.0, 0.25, 0.5))
    assert [r["maf_bin"] for r in custom] == ["[0,0.25)", "[0.25,0.5]", "ALL"] and [r["sites"] for r in custom] == [9, 3, n]
    none = aggregate(acc[:0], table[:0], maf[:0])
    assert none[-1]["sites"] == 0 and math.isnan(none[-1]["pooled_r2"])
    with pytest.raises(ValueError):
        aggregate(acc, table, maf, (0.0, 0.5, 0.1))


def test_accuracy_tsv_format():
    from src.quality import TSV_COLUMNS, accuracy_tsv
    rows = [dict(maf_bin="[0,0.5]", sites=3, genotypes=12, mean_r2=0.5, pooled_r2=float("nan"), concordance=1.0,
                 nonref_concordance=2 / 3)]
    text = accuracy_tsv(rows)
    assert text == "\t".join(TSV_COLUMNS) + "\n[0,0.5]\t3\t12\t0.500000\tnan\t1.000000\t0.666667\n"


def test_truth_maps():
    from src.quality import truth_maps
    tv = types.SimpleNamespace(pos=np.asarray([100, 200, 200, 300, 50], np.int32), samples=["c", "a", "x", "b"])
    ori = np.asarray([50, 100, 150, 200, 300])
    row, col = truth_maps(tv, ori, ["a", "b", "c"])
    assert row.dtype == col.dtype == np.int32
    assert row.tolist() == [4, 0, -1, 1, 3]                     # 200: the first of the two records
    assert col.tolist() == [1, 3, 0]                            # by name: reordered, one extra sample
    # a name the truth file lacks: the order fallback, which needs equal counts
    with pytest.raises(ValueError, match="4 samples"):
        truth_maps(tv, ori, ["a", "b", "zz"])
    row, col = truth_maps(tv, ori, ["a", "b", "zz", "c"])
    assert col.tolist() == [0, 1, 2, 3]
    row, col = truth_maps(tv, ori, n_samples=4)
    assert col.tolist() == [0, 1, 2, 3] and row.tolist() == [4, 0, -1, 1, 3]
    with pytest.raises(ValueError, match="4 samples"):
        truth_maps(tv, ori, n_samples=3)


def test_info_strings_format():
    from src.quality import info_strings
    got = info_strings(np.asarray([0.12345, 0.0, 1.0]), np.asarray([0.5, 0.0, 1.0]), np.asarray([0.25, 0.0, 0.99951]))
    assert got == ["AF=0.1235;DR2=0.250;R2=0.500;IMP", "AF=0.0000;DR2=0.000;R2=0.000;IMP", "AF=1.0000;DR2=1.000;R2=1.000;IMP"]


def test_host_writer_info_column_and_header(tmp_path):
    from src.infer_embedding_rag import write_vcf
    from src.vcf_device import header_lines, site_prefixes
    rng = np.random.default_rng(1)
    n, S = 5, 3
    h1, h2 = rng.random((n, S), dtype=np.float32), rng.random((n, S), dtype=np.float32)
    gt = (rng.random((n, S, 4), dtype=np.float32) / 4).astype(np.float32)
    pos = np.asarray([5, 17, 101, 2000, 30000])
    samples = ["A", "B", "C"]
    flag = np.asarray([1, 0, 1, 1, 0], bool)
    info = [f"AF=0.{i}000;DR2=0.5{i}0;R2=0.{i}25;IMP" for i in range(n)]
    args = (pos, h1, h2, gt, samples)
    write_vcf(tmp_path / "plain.vcf", "21", *args, pos_flag=flag)
    write_vcf(tmp_path / "none.vcf", "21", *args, pos_flag=flag, info=None)
    write_vcf(tmp_path / "info.vcf", "21", *args, pos_flag=flag, info=info)
    plain, with_info = (tmp_path / "plain.vcf").read_text(), (tmp_path / "info.vcf").read_text()
    assert (tmp_path / "none.vcf").read_text() == plain
    pl, il = plain.split("\n"), with_info.split("\n")
    added = [l for l in il if l not in pl and l.startswith("##")]
    assert len(il) == len(pl) + 4 and len(added) == 4
    assert [l.split(",")[0] for l in added] == ["##INFO=<ID=AF", "##INFO=<ID=DR2", "##INFO=<ID=R2", "##INFO=<ID=IMP"]
    assert il[2:6] == added and il[1] == "##source=rag-snvbert_amd"           # right behind the ##source line
    assert all("Number=1,Type=Float" in l for l in added[:3]) and "Number=0,Type=Flag" in added[3]
    body_p = [l for l in pl if l and not l.startswith("#")]
    body_i = [l for l in il if l and not l.startswith("#")]
    assert len(body_i) == 3
    for lp, li, i in zip(body_p, body_i, (0, 2, 3)):
        cp, ci = lp.split("\t"), li.split("\t")
        assert cp[7] == "." and ci[7] == info[i]                               # column 8 of the selected site rows
        assert cp[:7] == ci[:7] and cp[8:] == ci[8:]
    # the device writer's host-built pieces carry the same text
    assert header_lines(samples, True) == "\n".join(il[:11]) + "\n" and header_lines(samples) == "\n".join(pl[:7]) + "\n"
    rows, blob, off = site_prefixes("21", pos, flag, info=info, encoding="utf-8")
    assert rows.tolist() == [0, 2, 3]
    assert [blob[off[i]:off[i + 1]].decode() for i in range(3)] == [l[:l.index("GT:HDS:GP:DS\t") + 13] for l in body_i]
    with pytest.raises(ValueError):
        write_vcf(tmp_path / "bad.vcf", "21", *args, info=info[:2])


def test_flags_parse_and_default_off():
    from src import infer_embedding_rag as I
    a = I.parse_args([])
    assert a.vcf_info is False and a.truth_vcf is None and a.maf_bins is None
    a = I.parse_args(["--vcf_info", "--truth_vcf", "t.vcf.gz", "--maf_bins", "0,0.05,0.5"])
    assert a.vcf_info and a.truth_vcf == "t.vcf.gz"
    from src.quality import DEFAULT_MAF_EDGES, parse_maf_bins
    assert parse_maf_bins(a.maf_bins) == (0.0, 0.05, 0.5) and parse_maf_bins(None) == DEFAULT_MAF_EDGES
    assert DEFAULT_MAF_EDGES == (0.0, 0.001, 0.005, 0.01, 0.05, 0.1, 0.2, 0.5)


def test_synthetic_arrays_carry_the_truth():
    from src.dataset.synthetic import make_infer_arrays
    a = make_infer_arrays(300, 4, 12, missing_rate=0.5, seed=11)
    assert a["truth"].shape == (300, 4, 2) and a["truth"].dtype == np.int8
    keep = np.isin(a["ori_pos"], a["pos"])
    assert np.array_equal(a["truth"][keep], a["vcf"])           # the target is the truth at the sites it keeps
