"""Every instantiation of the block-tail family through the wrappers of src/kernels.py — tail_kernel<D,
PRE> (snvrag_tail_forward with tail_wide = 0, snvrag_tail_ffn_forward), tailw_body<G = 4 / 1, PROJ>
(snvrag_tail_forward with tail_wide = 1, snvrag_tail_qkv_forward), tail_kernel<D, false, NC> and
projw_kernel (snvrag_proj_forward) and the two stamped builds — against the fp64 references of
tests/tail_refs.py within their derived per-element bounds, on its input families and at the row
edges of its shape tables (tests/test_tail_refs_cpu.py proves the references, the bounds, their teeth
and the tables).

Every buffer a launch touches carries eight sentinel rows after row M: NaN in att, x (projection)
and x1, 7.0 in out, the in-place x and qkv_out.  Rows below M must be finite and within the bound,
the written sentinel rows unchanged bit for bit, and a second launch on the same inputs must give
the same bits.  max err / bound is printed per case.  The fp64 references run on the device, once
per (family, D, eps, entry) on the longest row count; every M is a row prefix (the function is
row-wise)."""
import contextlib

import pytest
import torch

import tail_refs as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F64 = torch.bfloat16, torch.float64
PADR = 8
SENT = 7.0
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cache():
    """The families' device operands and fp64 references (0.3 GB each at M_SPLIT) live for this module only."""
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def K():
    from src import kernels
    return kernels


def N():
    from src import native
    return native


@contextlib.contextmanager
def options(**kw):
    with contextlib.ExitStack() as st:
        for k, v in kw.items():
            st.enter_context(K().option(k, v))
        yield


def _guard(t, M, fill):
    """[M + 8, cols] device storage: the first M rows of t, then eight rows of fill."""
    buf = torch.full((M + PADR, t.shape[1]), fill, dtype=BF16, device=DEV)
    buf[:M] = t[:M]
    return buf


def _sentinel_ok(buf, M, what):
    tail = buf[M:]
    assert bool((tail == SENT).all()), f"{what}: wrote past row {M}"


def _same_bits(a, b, what):
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: two launches differ"


def _check(got, ref, bound, what):
    assert bool(torch.isfinite(got.float()).all()), f"{what}: not finite"
    r = T.ratio(got, ref, bound)
    print(f"{what}: max err/bound {r:.3f}")
    assert r <= 1.0, what
    return r


def _case(fam, D, eps=1e-5):
    """The family's operands on the device (weights packed once), Mmax rows."""
    key = ("case", fam, D, eps)
    if key not in _CACHE:
        c = T.case(fam, D, T.MMAX[D], eps)
        d = {k: getattr(c, k).to(DEV) for k in ("att", "x", "x1", "b_o", "g1", "be1", "vec")}
        d["ts"] = K().tail_pack(c.w_o.to(DEV), c.w1.to(DEV), c.w2g.to(DEV))
        d["c"] = c
        _CACHE[key] = d
    return _CACHE[key]


def _ref(fam, D, eps, pre):
    """out, bound, dout, fed_by_flag of the family on the device, Mmax rows (pre = False: the rows of
    tail_m(D) only)."""
    key = ("ref", fam, D, eps, pre)
    if key not in _CACHE:
        c = _case(fam, D, eps)["c"]
        r = T.ref_of(c, eps, pre, DEV, None if pre else T.rot_m(D))
        _CACHE[key] = {k: getattr(r, k) for k in ("out", "bound", "dout", "fed_by_flag")}
    return _CACHE[key]


def _qkv_weights():
    if "qkv" not in _CACHE:
        d = T.dense_proj(384, 3, 1)
        _CACHE["qkv"] = dict(w=d.w.to(DEV), b=d.b.to(DEV), pw=K().proj_pack(d.w.to(DEV)))
    return _CACHE["qkv"]


def run_tail(kind, d, M, eps, what):
    """Two guarded launches of 'tail' (snvrag_tail_forward), 'ffn' (snvrag_tail_ffn_forward) or 'qkv'
    (snvrag_tail_qkv_forward); (out [M, D], qkv [M, 3 D] or None) of the first."""
    res = []
    for _ in range(2):
        qkv = None
        if kind == "ffn":
            x1 = _guard(d["x1"], M, float("nan"))
            out = torch.full((M + PADR, x1.shape[1]), SENT, dtype=BF16, device=DEV)
            K().tail_ffn_forward(x1[:M], d["ts"], d["vec"], eps=eps, out=out[:M])
        else:
            att, out = _guard(d["att"], M, float("nan")), _guard(d["x"], M, SENT)
            if kind == "tail":
                K().tail_forward(att[:M], out[:M], d["ts"], d["b_o"], d["g1"], d["be1"], d["vec"], eps=eps)
            else:
                q = _qkv_weights()
                qkv = torch.full((M + PADR, 3 * 384), SENT, dtype=BF16, device=DEV)
                K().tail_qkv_forward(att[:M], out[:M], d["ts"], d["b_o"], d["g1"], d["be1"], d["vec"], q["pw"], q["b"],
                                     qkv_out=qkv[:M], eps=eps)
        res.append((out, qkv))
    torch.cuda.synchronize()
    for a, b in zip(*res):
        if a is not None:
            _same_bits(a, b, what)
            _sentinel_ok(a, M, what)
    out, qkv = res[0]
    return out[:M], None if qkv is None else qkv[:M]


def check_tail(kind, fam, D, M, eps, what):
    d = _case(fam, D, eps)
    r = _ref(fam, D, eps, kind != "ffn")
    out, qkv = run_tail(kind, d, M, T.f32(eps), what)
    worst = _check(out, r["out"][:M], r["bound"][:M], f"out {what}")
    if qkv is not None:
        # the projection of the kernel's own output rows, whose bf16 values are exact operands
        q = _qkv_weights()
        pr = T.proj_ref(out, q["w"], q["b"])
        worst = max(worst, _check(qkv, pr.out, pr.bound, f"qkv {what}"))
    return out, qkv, worst


def _family_cases(D, pre, ms_sparse, ms_other):
    fams = [("sparse", 1e-5)] + ([("phase_a", 1e-5)] if pre else []) + [("ln_rows", 1e-5), ("low_var", 1e-5), ("low_var", 1e-3)]
    return [(f, e, M) for f, e in fams for M in (ms_sparse if f == "sparse" else ms_other)]


# ------------------------------------------------------------------ tail_kernel --
@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("D", T.DS)
def test_tail_kernel_vs_fp64(D, pre):
    """tail_kernel<D, PRE> (tail_wide = 0): every M of the table on sparse; phase_a (PRE only), ln_rows
    and low_var (both eps) at M = 129 and at 128 NCH + 1 rows (every chunk rotation)."""
    name = f"tail_kernel<{D}, {'true' if pre else 'false'}>"
    with options(tail_wide=0, tail_variant=0):
        for fam, eps, M in _family_cases(D, pre, T.tail_m(D), (129, T.rot_m(D))):
            check_tail("tail" if pre else "ffn", fam, D, M, eps, f"{name} {fam} eps={eps} M={M}")


# ------------------------------------------------------------------- tailw_body --
@pytest.mark.parametrize("kind", ["tail", "qkv"])
@pytest.mark.parametrize("fam,eps", [("sparse", 1e-5), ("phase_a", 1e-5), ("ln_rows", 1e-5), ("low_var", 1e-5), ("low_var", 1e-3)])
def test_tail_wide_vs_fp64(fam, eps, kind):
    """tailw_body<4, PROJ> at every M of the wide-row table and, at M_SPLIT, the 32-row bodies
    tailw_body<1, PROJ> (tail_split = 64: the remainder as eight 32-row workgroups, the last with 5
    rows) and the unsplit launch (tail_split = 0).  kind = qkv: snvrag_tail_qkv_forward, whose qkv_out
    is checked with proj_ref on the kernel's own x rows."""
    name = f"tailw_body<G, {'true' if kind == 'qkv' else 'false'}>"
    with options(tail_wide=1, tail_variant=0):
        for M in T.WIDE_M:
            check_tail(kind, fam, 384, M, eps, f"{name} {fam} eps={eps} M={M}")
        for split in T.SPLITS:
            with options(tail_split=split):
                check_tail(kind, fam, 384, T.M_SPLIT, eps, f"{name} {fam} eps={eps} M={T.M_SPLIT} tail_split={split}")


# ------------------------------------------------------------------ projections --
@pytest.mark.parametrize("NC", [1, 3])
@pytest.mark.parametrize("D,wide", [(128, 0), (256, 0), (384, 0), (384, 1)])
def test_proj_vs_fp64(D, wide, NC):
    """tail_kernel<D, false, NC> (proj_wide = 0) and projw_kernel (D = 384, proj_wide = 1) on dense and
    sparse operands over the M table (128 NC + 1: every chunk rotation and a one-row tile; projw_kernel:
    and 160)."""
    name = "projw_kernel" if wide else f"tail_kernel<{D}, false, {NC}>"
    ms = T.proj_m(D, NC, bool(wide))
    for make in (T.dense_proj, T.sparse_proj):
        c = make(D, NC, max(ms))
        w, b = c.w.to(DEV), c.b.to(DEV)
        pw = K().proj_pack(w)
        full = T.proj_ref(c.x.to(DEV), w, b)
        for M in ms:
            what = f"{name} NC={NC} {make.__name__} M={M}"
            res = []
            for _ in range(2):
                x = _guard(c.x.to(DEV), M, float("nan"))
                out = torch.full((M + PADR, NC * D), SENT, dtype=BF16, device=DEV)
                with options(proj_wide=wide):
                    K().proj_forward(x[:M], pw, b, NC, out=out[:M])
                res.append(out)
            torch.cuda.synchronize()
            _same_bits(res[0], res[1], what)
            _sentinel_ok(res[0], M, what)
            _check(res[0][:M], full.out[:M], full.bound[:M], what)


# ---------------------------------------------------------------- stamped builds --
@contextlib.contextmanager
def stamps(M):
    """A snvrag_tail_stamps buffer as tools/tail_micro.py (workgroups x 4 waves x 10) and
    tools/tailw_diag.py (32-row workgroups x 4 waves x 8) size theirs, released with a null pointer."""
    st = torch.zeros(-(-M // 32) * 4 * 10, dtype=torch.int64, device=DEV)
    N().lib().snvrag_tail_stamps(st.data_ptr())
    try:
        yield st
    finally:
        torch.cuda.synchronize()
        N().lib().snvrag_tail_stamps(None)


STAMPED = [("tail_kernel<384, true, 0, true>", "tail", dict(tail_wide=0, tail_variant=4)),
           ("tail_kernel<384, false, 0, true>", "ffn", dict(tail_wide=0, tail_variant=4)),
           ("tailw_kernel<true>", "tail", dict(tail_wide=2, tail_variant=0)),
           ("tailw_kernel<true> qkv", "qkv", dict(tail_wide=2, tail_variant=0))]


@pytest.mark.parametrize("name,kind,opts", STAMPED, ids=[s[0] for s in STAMPED])
@pytest.mark.parametrize("M", [129, 3073])
def test_stamped_builds(M, name, kind, opts):
    """tail_kernel<384, PRE, 0, true> (both entries; reads 4 fragments ahead, not 8) and tailw_kernel<true>
    (with and without the projection), which only the tools/ micro-benchmarks launch: within the bound
    on sparse and bit-identical to the unstamped launch (the same arithmetic in the same order), out
    and qkv_out alike."""
    plain = dict(opts, tail_variant=0, tail_wide=min(opts["tail_wide"], 1))
    what = f"{name} sparse M={M}"
    with stamps(M) as st:
        with options(**opts):
            got, got_qkv, _ = check_tail(kind, "sparse", 384, M, 1e-5, f"{what} (stamped)")
        torch.cuda.synchronize()
        assert bool((st != 0).any()), "the stamped kernel did not run"
    with options(**plain):
        ref, ref_qkv = run_tail(kind, _case("sparse", 384), M, T.f32(1e-5), f"unstamped {kind} M={M}")
    _same_bits(got, ref, f"out, stamped vs unstamped {what}")
    assert (got_qkv is None) == (ref_qkv is None) == (kind != "qkv")
    if kind == "qkv":
        _same_bits(got_qkv, ref_qkv, f"qkv_out, stamped vs unstamped {what}")


# ------------------------------------------------------------------- cross-check --
def test_tailw_equals_tail_kernel_where_no_rounding_is_open():
    """sparse, M = 3073, D = 384: the two kernels sum in different orders, so they may differ only
    where a rounding is open — outputs a flagged x1 or hidden element feeds, and outputs whose fp64
    value lies within their own error bound of a bf16 midpoint.  Everywhere else both must give the
    bf16 rounding of the reference, bit for bit."""
    M = 3073
    d, r = _case("sparse", 384), _ref("sparse", 384, 1e-5, True)
    with options(tail_wide=1, tail_variant=0):
        a, _ = run_tail("tail", d, M, T.f32(1e-5), "tailw")
    with options(tail_wide=0, tail_variant=0):
        b, _ = run_tail("tail", d, M, T.f32(1e-5), "tail_kernel")
    closed = ~(r["fed_by_flag"][:M] | T.near_midpoint(r["out"][:M], r["dout"][:M]))
    share = float(closed.double().mean())
    diff = float((a != b).double().mean())
    print(f"tailw vs tail_kernel: {share:.4f} of the outputs compared bit for bit; {diff:.5f} of all outputs differ")
    assert share > 0
    assert torch.equal(a[closed].view(torch.int16), b[closed].view(torch.int16))
    assert torch.equal(a[closed].double(), T.rne_bf16(r["out"][:M])[closed])
