"""TK (reranker `TK`) on the host: the plugin's configuration and parameter surface against the reference's (fixtures made by
tests/golden/make_golden_tk.py from the reference TK_class), checkpoints, refusals, and the training restatement against the
reference's scores, features and gradients."""
import ctypes
import os

import numpy as np
import pytest
import torch

from capreolus_amd import reranker
from capreolus_amd.reranker import TK, TK_class
from tests import tk_case

REL = 1e-5


def _model(name):
    r, m = tk_case.build(name, TK)
    return r, m


def test_config_options_and_defaults():
    assert TK.module_name == "TK"
    assert TK.config_spec == {"gradkernels": True, "scoretanh": False, "singlefc": True, "projdim": 32, "ffdim": 100, "numlayers": 2,
                              "numattheads": 10, "alpha": 0.5, "usemask": False, "usemixer": False, "finetune": False}
    assert TK.supports_resident and not TK.supports_lists
    assert "TK" not in reranker.registry and reranker.TK is TK and reranker.TK_class is TK_class
    with pytest.raises(ValueError):
        TK({"nosuchoption": 1}, tk_case.extractor("tk_small"))


@pytest.mark.parametrize("name", list(tk_case.CASES))
def test_state_dict_names_and_shapes_match_the_reference(name):
    c = tk_case.load(name)
    _, m = _model(name)
    sd = m.state_dict()
    assert sorted(sd) == [str(k) for k in c["state_keys"]]
    for k, shape in zip(c["state_keys"], c["state_shapes"]):
        assert list(sd[str(k)].shape) == [int(x) for x in shape if x], k
    np.testing.assert_array_equal(m.position_encoder.pe[:16, 0].numpy(), c["pe_head"])


@pytest.mark.parametrize("name", list(tk_case.CASES))
def test_fixture_ids_are_what_tk_case_draws(name):
    """the fixtures' recorded ids are tk_case.inputs' (so its per-case options left the older cases' streams alone), with the edge
    patterns the kernels' tests rely on"""
    c = tk_case.load(name)
    q, d = tk_case.inputs(name)
    np.testing.assert_array_equal(c["query"], q)
    np.testing.assert_array_equal(c["posdoc"], d)
    assert (d == 0).any() and (q == 0).any() and (d == tk_case.ZERO_TOKEN).any() and (q == tk_case.ZERO_TOKEN).any()
    if tk_case.CASES[name].get("dead_tiles"):
        Z = tk_case.ZERO_TOKEN
        assert (d[4, :130] == Z).all() and d[4, 130] != Z and (d[5] == Z).all()
        assert (d[6] != Z).sum() == 1 and (d[6] != Z).argmax() > 128
        assert np.isin(q[6], (0, Z)).all()


def test_save_and_load_weights_round_trip(tmp_path):
    r, m = _model("tk_small")
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    fn = os.path.join(tmp_path, "w", "weights")
    r.save_weights(fn, opt)
    r2 = TK(tk_case.config("tk_small"), tk_case.extractor("tk_small"))
    m2 = r2.build_model()
    for p in m2.parameters():
        p.data.zero_()
    r2.load_weights(fn, torch.optim.Adam([p for p in m2.parameters() if p.requires_grad], lr=1e-3))
    a, b = m.state_dict(), m2.state_dict()
    assert set(a) == set(b)
    for k in a:
        if k != "embedding.weight":       # (not saved, as in the reference: it comes from the extractor)
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("cfg", [{"numattheads": 7}, {"numattheads": 0}, {"ffdim": 513}, {"ffdim": 0}, {"numlayers": 0}])
def test_unsupported_geometry_is_refused(cfg):
    with pytest.raises(ValueError):
        TK(dict(tk_case.config("tk_small"), **cfg), tk_case.extractor("tk_small")).build_model()
    ex = tk_case.extractor("tk_small")
    ex.embeddings = np.zeros((10, 520), dtype=np.float32)             # dim > 512
    with pytest.raises(ValueError):
        TK({"numattheads": 8}, ex).build_model()
    ex.embeddings = np.zeros((10, 130), dtype=np.float32)             # head width 65
    with pytest.raises(ValueError):
        TK({"numattheads": 2}, ex).build_model()


def test_abi_refuses_each_geometry_limit():
    """capamd_tk_workspace_bytes / capamd_tk_forward answer -1 / CAPAMD_ERR_ARG to what the kernels do not take (no device access)"""
    from capreolus_amd import _lib

    lib = _lib.load()
    P = 0x10000
    layers = (_lib.TkLayer * 3)(*[_lib.TkLayer(*([P] * 12)) for _ in range(3)])

    def model(**kw):
        m = _lib.TkModel()
        m.emb = m.pe = m.s_log_w = m.s_len_w = m.comb_w = P
        m.layers_host = ctypes.cast(layers, ctypes.c_void_p)
        m.vocab, m.pad, m.dim, m.heads, m.ffdim, m.numlayers, m.max_len, m.alpha, m.ln_eps = 1000, 0, 300, 10, 100, 2, 5000, 0.5, 1e-5
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert lib.capamd_tk_workspace_bytes(ctypes.byref(model()), 4, 4, 800) > 0
    bad = [({"dim": 513, "heads": 9}, {}), ({"heads": 7}, {}), ({"dim": 130, "heads": 2}, {}), ({"ffdim": 513}, {}), ({"ffdim": 0}, {}),
           ({"numlayers": 0}, {}), ({"heads": 0}, {}), ({"max_len": 100}, {}), ({}, {"Q": 33}), ({}, {"Q": 0}), ({}, {"L": 5001}), ({}, {"L": 0}),
           ({}, {"nb": 0})]
    for mkw, skw in bad:
        m = model(**mkw)
        Q, L, nb = skw.get("Q", 4), skw.get("L", 800), skw.get("nb", 4)
        assert lib.capamd_tk_workspace_bytes(ctypes.byref(m), nb, Q, L) == -1, (mkw, skw)
        assert lib.capamd_tk_forward(P, P, 8, Q, L, ctypes.byref(m), nb, P, 1 << 40, P, None, P, None) == _lib.ERR_ARG, (mkw, skw)
    # a missing layer tensor is refused too
    layers[1].w2 = None
    assert lib.capamd_tk_forward(P, P, 8, 4, 800, ctypes.byref(model()), 4, P, 1 << 40, P, None, P, None) == _lib.ERR_ARG


@pytest.mark.parametrize("name", tk_case.SCORE_CASES)
def test_restatement_matches_the_reference(name):
    c = tk_case.load(name)
    _, m = _model(name)
    m.eval()
    with torch.no_grad():
        score, feats = m._forward_aten(torch.from_numpy(c["posdoc"]), torch.from_numpy(c["query"]), return_features=True)
    want = np.concatenate([c["s_log_k"], c["s_len_k"]], axis=1)
    scale = np.abs(want).max(axis=1, keepdims=True)
    assert np.abs(feats.numpy() - want).max() <= REL * scale.max(), np.abs(feats.numpy() - want).max()
    assert np.all(np.abs(feats.numpy() - want) <= REL * scale)
    np.testing.assert_allclose(score.numpy(), c["score"], rtol=REL, atol=REL * np.abs(c["score"]).max())
    assert np.all(np.isfinite(score.numpy()))


def test_restatement_gradients_match_the_reference():
    c = tk_case.load("tk_grad")
    _, m = _model("tk_grad")
    m.train()
    m.position_encoder.dropout.p = 0.0
    score = m(torch.from_numpy(c["posdoc"]), torch.from_numpy(c["query"]), None).view(-1)
    np.testing.assert_allclose(score.detach().numpy(), c["score"], rtol=REL, atol=REL * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"])).sum().backward()
    names = [k[len("grad."):] for k in c if k.startswith("grad.")]
    assert set(names) == {k for k, p in m.named_parameters() if p.requires_grad}
    params = dict(m.named_parameters())
    for k in names:
        want, got = c["grad." + k], params[k].grad.numpy()
        assert np.abs(got - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6), (k, np.abs(got - want).max(), np.abs(want).max())


def test_dropout_applies_to_x_plus_pe_in_training_mode_only():
    _, m = _model("tk_small")
    c = tk_case.load("tk_small")
    d, q = torch.from_numpy(c["posdoc"][:2]), torch.from_numpy(c["query"][:2])
    seen = []
    h = m.position_encoder.dropout.register_forward_hook(lambda mod, inp, out: seen.append((mod.training, inp[0].detach(), out.detach())))
    m.train()
    torch.manual_seed(1)
    m(d, q, None)
    assert seen and all(t for t, _, _ in seen)
    _, x, y = seen[0]
    emb = m.embedding(d)
    torch.testing.assert_close(x, emb + m.position_encoder.pe[: d.shape[1], 0].unsqueeze(0), rtol=0, atol=0)
    dropped = (y == 0) & (x != 0)
    assert 0.05 < dropped.float().mean().item() < 0.15
    torch.testing.assert_close(y[~dropped], x[~dropped] / 0.9)
    m.eval()
    seen.clear()
    with torch.no_grad():
        m._forward_aten(d, q)
    _, x, y = seen[0]
    assert torch.equal(x, y)
