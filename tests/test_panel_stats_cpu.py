"""The host side of the panel tables (src/dataset/panel_stats.py, src/build_panel_stats.py): the count
specification against a hand-written table and an independent loop, the quotients, the sample / population
bookkeeping with its errors, the files' round trip into InferDataset, and the refused flag combinations."""
import pickle

import numpy as np
import pytest

from src.dataset import panel_stats as PS


# 4 sites x 5 samples; populations A, B interleaved (s0 A, s1 B, s2 A, s3 B, s4 A)
M = -1
GT = np.array([
    [[0, 0], [0, 1], [1, 1], [2, 0], [M, M]],       # a 2|0 and a missing call
    [[M, 1], [0, 0], [0, 0], [1, 1], [1, 0]],       # a half-missing call
    [[M, M], [M, M], [M, M], [M, M], [M, M]],       # nothing called
    [[1, M], [M, 0], [0, 1], [0, 0], [1, 1]],       # two haploid calls
], np.int8)
ORDER, POP_START = np.array([0, 2, 4, 1, 3], np.int32), np.array([0, 3, 5], np.int32)
# columns n_ref, n_het, n_hom, n_alt, n_called per site
WANT_A = [[1, 0, 1, 2, 4], [1, 1, 0, 2, 5], [0, 0, 0, 0, 0], [0, 1, 1, 4, 5]]
WANT_B = [[0, 2, 0, 2, 4], [1, 0, 1, 2, 4], [0, 0, 0, 0, 0], [1, 0, 0, 0, 3]]
WANT_G = [[1, 2, 1, 4, 8], [2, 1, 1, 4, 9], [0, 0, 0, 0, 0], [1, 1, 1, 4, 8]]


def test_counts_of_the_hand_written_table():
    got = PS.panel_counts_host(GT, ORDER, POP_START, 2)
    assert got.dtype == np.int32 and got.shape == (6, 5, 4)
    np.testing.assert_array_equal(got[0].T, WANT_A)
    np.testing.assert_array_equal(got[1].T, WANT_B)
    np.testing.assert_array_equal(got[5].T, WANT_G)
    assert not got[2:5].any()


def loop_counts(gt, order, pop_start, P):
    out = np.zeros((6, 5, gt.shape[0]), np.int32)
    for p in range(P):
        for s in order[pop_start[p]:pop_start[p + 1]]:
            for r in range(gt.shape[0]):
                a, b = int(gt[r, s, 0]), int(gt[r, s, 1])
                for row in (p, 5):
                    if a >= 0 and b >= 0:
                        out[row, (a > 0) + (b > 0), r] += 1
                    out[row, 3, r] += (a > 0) + (b > 0)
                    out[row, 4, r] += (a >= 0) + (b >= 0)
    return out


def random_case(n, S, P, seed, missing=0.1):
    """gt int8 [n, S, 2] with allele numbers 0..3 and ``missing`` of the alleles -1; populations interleaved in
    sample order (sample s in population s % P; when S allows, population 0 is the last sample alone)."""
    rng = np.random.default_rng(seed)
    gt = rng.choice(np.array([0, 0, 0, 1, 1, 2, 3], np.int8), (n, S, 2))
    gt[rng.random((n, S, 2)) < missing] = -1
    key = np.arange(S) % P
    if S > P:
        key[key == 0] = 1 % P
        key[S - 1] = 0
    order = np.argsort(key, kind="stable").astype(np.int32)
    pop_start = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=P))]).astype(np.int32)
    return gt, order, pop_start


@pytest.mark.parametrize("n,S,P", [(17, 9, 1), (40, 23, 2), (33, 31, 5)])
def test_counts_against_an_independent_loop(n, S, P):
    gt, order, pop_start = random_case(n, S, P, seed=n + S)
    assert (order != np.arange(S)).any() or P == 1
    got = PS.panel_counts_host(gt, order, pop_start, P)
    np.testing.assert_array_equal(got, loop_counts(gt, order, pop_start, P))
    assert not got[P:5].any()
    np.testing.assert_array_equal(got[5], got[:5].sum(0))


def test_freq_from_counts():
    gt, order, pop_start = random_case(200, 37, 3, seed=5, missing=0.3)
    gt[7] = -1                                               # nothing called: every denominator 0
    gt[8, :, 1] = -1                                         # haploid only: no genotype, AF defined
    counts = PS.panel_counts_host(gt, order, pop_start, 3)
    f = PS.freq_from_counts(counts)
    assert f.dtype == np.float32 and f.shape == (4, 6, 200)
    assert np.isfinite(f).all() and (f >= 0).all() and (f <= 1).all()
    assert not f[:, :, 7].any() and not f[:3, :, 8].any() and f[3, 5, 8] > 0
    assert not f[:, 3:5].any()                               # the unused population rows
    c = counts.astype(np.float64)
    geno = c[:, 0] + c[:, 1] + c[:, 2]
    ok = geno > 0
    total = f[0].astype(np.float64) + f[1] + f[2]
    assert (np.abs(total[ok] - 1) <= 2 * np.finfo(np.float32).eps).all()
    assert not total[~ok].any()
    # layer and row order, each quotient rounded once from float64
    for layer, num in enumerate((c[:, 0], c[:, 1], c[:, 2])):
        np.testing.assert_array_equal(f[layer][ok], (num[ok] / geno[ok]).astype(np.float32))
    ok = c[:, 4] > 0
    np.testing.assert_array_equal(f[3][ok], (c[:, 3][ok] / c[:, 4][ok]).astype(np.float32))
    np.testing.assert_array_equal(PS.freq_from_counts(PS.panel_counts_host(GT, ORDER, POP_START, 2))[:, 5, 0],
                                  np.array([1 / 4, 2 / 4, 1 / 4, 4 / 8], np.float32))


def test_population_order_and_maps():
    names = ["x9", "s3", "s0", "s1", "s2", "s4"]             # the panel file's own order, one sample not in the VCF
    pops = ["ZZZ", "EUR", "EUR", "AFR", "EUR", "AFR"]
    vcf = ["s0", "s1", "s2", "s3", "s4"]
    pop_list, order, pop_start = PS.population_order(vcf, names, pops)
    assert pop_list == ["AFR", "EUR"]                        # ZZZ belongs to no VCF sample
    assert order.dtype == pop_start.dtype == np.int32
    np.testing.assert_array_equal(order, [1, 4, 0, 2, 3])    # stable inside a population
    np.testing.assert_array_equal(pop_start, [0, 2, 5])
    with pytest.raises(ValueError, match="'s7'"):
        PS.population_order(["s0", "s7", "s8"], names, pops)
    with pytest.raises(ValueError, match="'s1'.*twice"):
        PS.population_order(vcf, names + ["s1"], pops + ["EUR"])
    six = [f"P{i}" for i in range(6)]
    with pytest.raises(ValueError, match="row 5 .*Global"):
        PS.population_order(six, six, six)
    PS.population_order(six[:5], six, six)

    pop_to_idx, pos_to_idx = PS.maps(pop_list, np.array([30, 10, 20], np.int32))
    assert pop_to_idx == {"AFR": 0, "EUR": 1, "Global": 5}
    assert list(pos_to_idx.items()) == [(30, 0), (10, 1), (20, 2)]
    assert all(type(k) is int for k in pos_to_idx)
    with pytest.raises(ValueError, match="POS 20 "):
        PS.maps(pop_list, [10, 20, 30, 20, 10])


def test_read_panel_file(tmp_path):
    path = tmp_path / "p.panel"
    path.write_text("sample\tpop\tsuper_pop\tgender\nA1\tGBR\tEUR\tmale\nA2\tYRI\tAFR\tfemale\n\n")
    assert PS.read_panel_file(path) == (["A1", "A2"], ["EUR", "AFR"])
    path.write_text("sample\tpop\tsuper_pop\nA1\tGBR\n")
    with pytest.raises(ValueError, match="line 2"):
        PS.read_panel_file(path)


def test_files_round_trip_into_infer_dataset(tmp_path):
    from src.build_panel_stats import FILES, write_tables
    from src.dataset.dataset import InferDataset, PanelData
    from src.dataset.vocab import WordVocab
    gt, order, pop_start = random_case(50, 12, 2, seed=9)
    pos = (np.arange(50) * 7 + 100).astype(np.int32)
    pos[[3, 4]] = pos[[4, 3]]                                # file order, not sorted order
    counts = PS.panel_counts_host(gt, order, pop_start, 2)
    pop_to_idx, pos_to_idx = PS.maps(["AFR", "EUR"], pos)
    tables = dict(freq=PS.freq_from_counts(counts), pop_to_idx=pop_to_idx, pos_to_idx=pos_to_idx, type_to_idx={},
                  counts=counts)
    paths = write_tables(tables, tmp_path / "out")
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(FILES.values())
    loaded = {}
    for k in ("pop_to_idx", "pos_to_idx", "type_to_idx"):
        with open(paths[k], "rb") as f:
            loaded[k] = pickle.load(f)
    assert loaded == dict(pop_to_idx=pop_to_idx, pos_to_idx=pos_to_idx, type_to_idx={})
    freq = np.load(paths["freq"])
    np.testing.assert_array_equal(freq, tables["freq"])
    np.testing.assert_array_equal(np.load(paths["counts"]), counts)
    target = (gt[::2, :3] > 0).astype(np.int8)
    ds = InferDataset(WordVocab(["AFR", "EUR"]), target, pos[::2], PanelData(["EUR", "AFR", "EUR"]), freq,
                      loaded["type_to_idx"], loaded["pop_to_idx"], loaded["pos_to_idx"])
    np.testing.assert_array_equal(ds.ori_pos, pos)
    item = ds[0]
    np.testing.assert_array_equal(item["af"][1:51].numpy(), freq[3, 5])      # behind the start token's slot
    np.testing.assert_array_equal(item["af_p"][1:51].numpy(), freq[3, 1])


FILES_ARGS = ["--infer_dataset", "t.vcf", "--infer_panel", "t.panel"]


@pytest.mark.parametrize("extra", [
    ["--ref_panel", "p.vcf", "--ref_panel_pops", "p.panel", "--freq_path", "f.npy"],
    ["--ref_panel", "p.vcf", "--ref_panel_pops", "p.panel", "--pop_path", "f.bin"],
    ["--ref_panel", "p.vcf", "--ref_panel_pops", "p.panel", "--pos_path", "f.bin"],
    ["--ref_panel", "p.vcf", "--ref_panel_pops", "p.panel", "--type_path", "f.bin"],
    ["--ref_panel", "p.vcf", "--ref_panel_pops", "p.panel", "--synthetic", "4"],
    ["--ref_panel_pops", "p.panel"],
    ["--ref_panel", "p.h5", "--ref_panel_pops", "p.panel"],
])
def test_parse_args_refuses(extra, capsys):
    from src.infer_embedding_rag import parse_args
    with pytest.raises(SystemExit):
        parse_args(FILES_ARGS + extra)
    assert "--ref_panel_pops" in capsys.readouterr().err


def test_parse_args_accepts_the_flag_and_its_absence():
    from src.infer_embedding_rag import parse_args
    a = parse_args(FILES_ARGS + ["--ref_panel", "p.vcf.gz", "--ref_panel_pops", "p.panel"])
    assert a.ref_panel_pops == "p.panel" and a.freq_path is None
    assert parse_args(FILES_ARGS + ["--ref_panel", "p.h5", "--freq_path", "f.npy"]).ref_panel_pops is None
    from src.build_panel_stats import parse_args as tool_args
    t = tool_args(["--ref_panel", "p.vcf", "--ref_panel_pops", "p.panel", "-o", "out", "--vcf_inflate", "device"])
    assert (t.output_dir, t.vcf_inflate) == ("out", "device")
    with pytest.raises(SystemExit):
        tool_args(["--ref_panel", "p.h5", "--ref_panel_pops", "p.panel", "-o", "out"])
