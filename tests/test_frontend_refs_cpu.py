"""The float64 restatements of tests/frontend_refs.py agree with their oracle/model_np.py
counterparts on the weights and inputs of the fwd_tiny golden: this ties the references of the
kernel-level tests (test_gpu_frontend_kernels.py) to the ones the goldens were validated against."""

import numpy as np
import pytest
import torch

import frontend_refs as R
from conftest import golden_state_dict, load_golden
from oracle import model_np

TOL = dict(rtol=1e-5, atol=1e-5)


@pytest.fixture(scope="module")
def tiny():
    g = load_golden("fwd_tiny")
    return g, golden_state_dict(g["cfg"])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_af_features_vs_oracle(tiny):
    g, sd = tiny
    fr = sd["bert.embedding.af_embedding.basis_freqs"]
    got = R.af_features(_t(g["af"]), _t(fr))
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), model_np.af_features(g["af"], fr), **TOL)


def test_embed_vs_oracle(tiny):
    g, sd = tiny
    afemb = model_np.af_embedding(g["af"], sd)                       # [B, L, D]
    W, pe = sd["bert.embedding.tokenizer.weight"], sd["bert.embedding.position.pe"][0]
    B = g["af"].shape[0]
    for key in ("hap_1", "hap_2"):
        got = R.embed(_t(g[key]), _t(W), _t(pe), _t(afemb), 0)
        np.testing.assert_allclose(got.numpy(), model_np.embed(g[key], g["af"], sd), **TOL)
    # the engine's layout: both haplotypes stacked, afemb rows shared with period B
    tok = np.concatenate([g["hap_1"], g["hap_2"]])
    ref = np.concatenate([model_np.embed(g["hap_1"], g["af"], sd), model_np.embed(g["hap_2"], g["af"], sd)])
    np.testing.assert_allclose(R.embed(_t(tok), _t(W), _t(pe), _t(afemb), B).numpy(), ref, **TOL)
    np.testing.assert_allclose(R.embed(_t(g["hap_1"]), _t(W), _t(pe), _t(afemb), 0).numpy(), g["emb_h1"], **TOL)


def _posfeat_w(sd, p="bert.emb_fusion.pos_feat"):
    names = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias",
             "norm1.weight", "norm1.bias", "norm1.running_mean", "norm1.running_var",
             "norm2.weight", "norm2.bias", "norm2.running_mean", "norm2.running_var")
    return [_t(sd[f"{p}.{n}"]) for n in names]


def test_posfeat_vs_oracle(tiny):
    g, sd = tiny
    got = R.posfeat(_t(g["pos"]), _posfeat_w(sd), model_np.EPS)
    np.testing.assert_allclose(got.numpy(), model_np.pos_feat(g["pos"], sd), **TOL)
    np.testing.assert_allclose(got.numpy(), g["posfeat"], **TOL)


def test_af_gate_vs_oracle(tiny):
    g, sd = tiny
    q = "bert.rag_fusion.af_interaction"
    w = [_t(sd[f"{q}.{n}"]) for n in ("gate_net.0.weight", "gate_net.0.bias", "gate_net.2.weight", "gate_net.2.bias",
                                      "joint_encoder.0.weight", "joint_encoder.0.bias",
                                      "joint_encoder.1.weight", "joint_encoder.1.bias")]
    got = R.af_gate(_t(g["af"]), _t(g["af_p"]), w, float(sd[q + ".res_scale"]))
    np.testing.assert_allclose(got.numpy(), model_np.af_interaction(g["af"], g["af_p"], sd), **TOL)


def test_rag_concat_is_the_oracle_weighting(tiny):
    """rag_fusion's `rag * w` and cat(orig, .) on golden activations (period = rows of one set)."""
    g, _ = tiny
    q, r = g["h1_before"], g["rag_mean_h1"]
    rng = np.random.default_rng(0)
    wgt = rng.random(q.shape[1:], dtype=np.float32)                   # [L, D], shared by the B rows
    got = R.rag_concat(_t(q), _t(r), _t(wgt), q.shape[1]).reshape(*q.shape[:2], -1)
    ref = np.concatenate([q, (r * wgt[None]).astype(np.float32)], -1)
    np.testing.assert_allclose(got.numpy(), ref, **TOL)


def test_hap_head_vs_oracle(tiny):
    g, sd = tiny
    h = model_np.hap_hidden(g["h1_after"], g["af"], g["af_p"], sd)
    logits, probs = R.hap_head(_t(h), _t(sd["hap_classifier.net.2.weight"]), _t(sd["hap_classifier.net.2.bias"]))
    ol, op = model_np.hap_head(g["h1_after"], g["af"], g["af_p"], sd)
    np.testing.assert_allclose(logits.numpy(), ol, **TOL)
    np.testing.assert_allclose(probs.numpy(), op, **TOL)
    np.testing.assert_allclose(logits.numpy(), g["logits_h1"], rtol=1e-4, atol=1e-4)


def test_gt_head_vs_oracle(tiny):
    g, sd = tiny
    p = "gt_classifier"
    w = [_t(sd[f"{p}.{n}"]) for n in ("gf_fusion.weight", "gf_fusion.bias", "gf_norm.weight", "gf_norm.bias",
                                      "layer.w_1.weight", "layer.w_1.bias", "layer.norm.weight", "layer.norm.bias",
                                      "layer.w_2.weight", "layer.w_2.bias", "classifier.weight", "classifier.bias")]
    B, L = g["ref"].shape
    got = R.gt_head(_t(g["probs_h1"]), _t(g["probs_h2"]), _t(g["ref"]), _t(g["het"]), _t(g["hom"]), 0, w)
    ref = model_np.gt_head(g["probs_h1"], g["probs_h2"], g["ref"], g["het"], g["hom"], sd)
    np.testing.assert_allclose(got.numpy().reshape(B, L, 4), ref, **TOL)
    np.testing.assert_allclose(got.numpy().reshape(B, L, 4), g["gt"], **TOL)
    # period: one set of side rows shared by two stacked copies of the batch
    two = R.gt_head(_t(np.concatenate([g["probs_h1"]] * 2)), _t(np.concatenate([g["probs_h2"]] * 2)),
                    _t(g["ref"]), _t(g["het"]), _t(g["hom"]), B * L, w)
    np.testing.assert_allclose(two.numpy().reshape(2, B, L, 4)[1], ref, **TOL)
