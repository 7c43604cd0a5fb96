"""The deterministic training mode's plumbing, without a GPU: the ``--deterministic`` flag reaches
the trainer keyword (default off), and the header declares / ``native.py`` binds every fixed-order
entry point the mode calls."""

import re
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]

NEW_EXPORTS = ("snvrag_linear_dw_det_ws_bytes", "snvrag_linear_dw_det", "snvrag_linear_dw_parts_det",
               "snvrag_nbr_mean_drop_bwd_det_ws_bytes", "snvrag_nbr_mean_drop_bwd_det",
               "snvrag_focal_loss_det_ws_bytes", "snvrag_focal_loss_det")


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.bert = torch.nn.Module()
        self.bert.embedding = torch.nn.Module()


def _trainer(argv):
    from src import train_embedding_rag as T
    from src.main.pretrain_with_val_optimized import BERTTrainerWithValidationOptimized
    args = T.parse_args(argv)
    return args, BERTTrainerWithValidationOptimized(_Stub(), None, None, None, **T.trainer_kwargs(args))


def test_flag_parses_and_reaches_the_trainer_keyword():
    args, tr = _trainer(["--deterministic", "--lr", "1e-3"])
    assert args.deterministic is True and tr.deterministic is True
    assert tr.optim.param_groups[0]["lr"] is not None      # the other arguments keep their meaning
    assert args.lr == 1e-3 and args.dims == 384


def test_default_is_off():
    import inspect
    from src.main.pretrain_with_val_optimized import BERTTrainerWithValidationOptimized
    args, tr = _trainer([])
    assert args.deterministic is False and tr.deterministic is False
    assert inspect.signature(BERTTrainerWithValidationOptimized.__init__).parameters["deterministic"].default is False
    assert BERTTrainerWithValidationOptimized(_Stub()).deterministic is False


def test_header_declares_every_new_export():
    header = (REPO / "include" / "snvrag.h").read_text()
    declared = set(re.findall(r"\b(snvrag_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_EXPORTS) <= declared, set(NEW_EXPORTS) - declared
    assert "deterministic" in header                        # the option is documented with the others


def test_native_binds_every_new_export():
    from src import native
    assert set(NEW_EXPORTS) <= set(native.EXPORTED), set(NEW_EXPORTS) - set(native.EXPORTED)
    for name in NEW_EXPORTS:
        args, res = native._SIGS[name]
        if name.endswith("_ws_bytes"):
            assert res is native.sz
        else:
            # a caller-owned workspace: (ws, ws_bytes) in front of the stream
            assert res is native.C.c_int and args[-3:] == [native.vp, native.sz, native.vp], name
