"""The entry points' argument checks: one refused call per row of tests/golden/arg_errors.json.

The rows [entry, case, message] were recorded from the library before its checks moved onto the
shared helpers of csrc/host.h (SNV_CHECK_PTRS / SNV_CHECK_ALIGN / SNV_CHECK_M); every call must
still be refused with exactly that text.  A case names the one argument that is wrong:
``null@i`` (argument i is a null pointer), ``misaligned@i`` (a real tensor, 2 bytes past its start),
``M@i`` (2^31 rows) and ``D@i`` (a width of 100).  The text is pinned whole, with the name before the
colon: the entry's own, or that of the helper that checks on its behalf (``dw_check`` and the like).
Every call returns before any launch, so no kernel runs, and the tensors passed in must come back
untouched.
"""
import ctypes as C
import json
import re
import sys
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "rag-snvbert_amd"))
from src import native  # noqa: E402

ROWS = [tuple(r) for r in json.loads((REPO / "tests" / "golden" / "arg_errors.json").read_text())]
SLOT = 256            # bytes per pointer argument, each at a 256-byte boundary of one buffer
FILL = 0xA5

# integer arguments that are not 0 in the otherwise valid call (argument index -> value), so that
# the checks before the one under test pass.  Where an entry returns at once on an empty batch,
# before it checks anything, the batch is 1; everywhere else it stays 0, which returns after the checks
_GEMM = {0: 1, 1: 1, 3: 64, 4: 64, 6: 64, 8: 64, 10: 64}
_DW = {1: 128, 2: 128, 4: 128, 6: 128}
_NBR = {1: 1, 2: 2, 3: 2, 6: 4}
BASE = {
    "snvrag_tail_forward": {1: 384}, "snvrag_tail_ffn_forward": {1: 384}, "snvrag_tail_qkv_forward": {1: 384},
    "snvrag_tail_pack": {0: 384}, "snvrag_proj_pack": {0: 384, 1: 3}, "snvrag_proj_forward": {1: 384, 2: 3},
    "snvrag_sgemm_pack": {0: 384, 1: 384}, "snvrag_sgemm_forward": {1: 384, 2: 384, 11: 1},
    "snvrag_sgemm_cat_forward": {1: 384, 2: 384, 6: 1}, "snvrag_mlp_pack": {0: 384},
    "snvrag_mlp_forward": {1: 384, 8: 1}, "snvrag_mlp_afgate_forward": {1: 384},
    "snvrag_gemm256_forward": {1: 384, 2: 64, 4: 64, 8: 384, 10: 384},
    "snvrag_gemm256_ln_forward": {1: 384, 2: 64, 4: 64, 11: 384, 16: 384},
    "snvrag_linear": _GEMM, "snvrag_linear_ex": _GEMM,
    "snvrag_linear_dw": _DW, "snvrag_linear_dw_parts": _DW, "snvrag_linear_dw_parts_det": _DW,
    "snvrag_linear_dw_det": {**_DW, 0: 1, 9: 1, 11: 1 << 40},
    "snvrag_knn_scan": {2: 256, 3: 256, 6: 2, 7: 4, 10: 1}, "snvrag_knn_scan_bits": {2: 32, 3: 256, 6: 2, 7: 4, 10: 1},
    "snvrag_knn_emb_pack": {1: 64, 2: 64}, "snvrag_knn_emb_scan": {1: 64, 2: 64, 4: 1, 5: 1},
    "snvrag_neighbor_counts": {1: 1, 4: 16, 8: 16}, "snvrag_neighbor_counts_bits": {1: 1, 4: 2, 8: 16},
    "snvrag_panel_pack_bits": {1: 1, 2: 16, 4: 2}, "snvrag_panel_unpack_rows": {2: 2, 4: 1, 6: 16},
    "snvrag_nbr_mean_drop_fwd": _NBR, "snvrag_nbr_mean_drop_bwd": _NBR, "snvrag_nbr_mean_drop_bwd_det": _NBR,
    "snvrag_vcf_format": {0: 1, 1: 1}, "snvrag_site_stats": {0: 1, 1: 1},
    "snvrag_vcf_line_index": {1: 16}, "snvrag_vcf_parse_gt": {1: 16, 4: 1, 9: 4},
    "snvrag_vcf_pack_rows": {1: 4, 3: 1, 7: 8},
    "snvrag_bgzf_inflate": {4: 1}, "snvrag_bgzf_deflate": {2: 1},
    # (nq = 1, limbs = 1: the float4 alignment check comes after the empty-batch return, and limbs = 2 clears a tail first)
    "snvrag_knn_lut_panel": {0: 1, 1: 2, 2: 4, 15: 1}, "snvrag_tokgrad": {0: 1, 1: 1, 2: 2}, "snvrag_head2_fwd": {0: 1, 1: 8}, "snvrag_head2_bwd": {0: 1, 1: 8, 9: 1 << 40},
    "snvrag_sqnorm_ws": {4: 1 << 20}, "snvrag_batch_features": {4: 8},
}
# a host structure argument is all zeros, except: every pointer field set, and these integer fields
STRUCT_FIELDS = {"snvrag_batch_features": dict(ld_bits=1, n_cols=1, n_samples=1, n_windows=1, n_pop=1)}


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def call(lib, buf, entry, case):
    """Make the call ``case`` of ``entry``: valid arguments but the one the case names."""
    kind, at = case.split("@")
    at = int(at)
    argtypes, _ = native._SIGS[entry]
    keep, args = [], []
    for i, t in enumerate(argtypes):
        if t is C.c_char_p:
            v = b""
        elif t is C.c_void_p:
            v = buf[i * SLOT:].data_ptr()
        elif _is_pointer(t):                       # a host structure or a host pointer array: zeros
            keep.append((t._type_ * 4)() if t._type_ is C.c_void_p else t._type_())
            v = keep[-1]
            if entry in STRUCT_FIELDS:
                for name, ft in v._fields_:
                    setattr(v, name, buf.data_ptr() if ft is C.c_void_p else STRUCT_FIELDS[entry].get(name, 0))
        elif t is C.c_float:
            v = 0.0
        else:
            v = BASE.get(entry, {}).get(i, 0)
        if i == at:
            assert (kind in ("null", "misaligned")) == (t is C.c_void_p), (entry, case)
            v = {"null": None, "misaligned": buf[i * SLOT + 2:].data_ptr(), "M": 1 << 31, "D": 100}[kind]
        args.append(v)
    rc = getattr(lib, entry)(*args)
    return rc, lib.snvrag_last_error().decode()


def test_fixture_covers_the_four_kinds():
    kinds = {case.split("@")[0] for _, case, _ in ROWS}
    assert kinds == {"null", "misaligned", "M", "D"}
    assert len(ROWS) == len({(e, c) for e, c, _ in ROWS}) >= 100
    # a check's text under the entry's name, or under that of the helper that checks for it
    helpers = {"snvrag_linear_ex", "dw_check", "launch_dw_det", "sqnorm_impl", "nbr_args", "rag_mean_launch"}
    assert all(m.split(": ")[0] in helpers | {e} for e, _, m in ROWS)
    assert set(BASE) | set(STRUCT_FIELDS) <= {e for e, _, _ in ROWS}


def _entry_bodies():
    """name -> body text of every extern "C" int entry point of csrc/*.hip (braces matched)."""
    out = {}
    for path in sorted((REPO / "rag-snvbert_amd" / "csrc").glob("*.hip")):
        text = path.read_text()
        for m in re.finditer(r'extern "C" int (snvrag_\w+)\([^)]*\)\s*\{', text):
            depth, i = 1, m.end()
            while depth:
                depth += {"{": 1, "}": -1}.get(text[i], 0)
                i += 1
            out[m.group(1)] = text[m.end():i]
    return out


def test_every_entry_on_the_shared_checks_has_rows():
    # an entry point whose own body uses the shared checks has a row; one that checks an alignment a
    # 2-byte offset can violate (more than 2 bytes) has a misaligned row; one with SNV_CHECK_M an M row
    kinds = {}
    for e, case, _ in ROWS:
        kinds.setdefault(e, set()).add(case.split("@")[0])
    missing = []
    for name, body in _entry_bodies().items():
        want = set()
        if "SNV_CHECK_PTRS(" in body:
            want.add("null")
        if "SNV_CHECK_M(" in body:
            want.add("M")
        if any(int(n) > 2 for n in re.findall(r"(?:SNV_CHECK_ALIGN|aligned)\((\d+),", body)):
            want.add("misaligned")
        if not want <= kinds.get(name, set()):
            missing.append((name, sorted(want - kinds.get(name, set()))))
    assert missing == []


@pytest.mark.gpu
def test_refused_calls_give_the_recorded_text():
    lib = native.load()
    buf = torch.full((32 * SLOT,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % SLOT == 0
    ref = buf.clone()
    torch.cuda.synchronize()
    bad = []
    for entry, case, message in ROWS:
        rc, text = call(lib, buf, entry, case)
        if rc == 0 or text != message:
            bad.append((entry, case, rc, text, message))
    torch.cuda.synchronize()
    assert bad == []
    assert torch.equal(buf, ref), "a refused call wrote to a tensor it was passed"
