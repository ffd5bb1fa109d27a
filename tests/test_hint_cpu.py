"""HINT (reranker `HINT`) on the host: the plugin's configuration and parameter surface against the reference's (fixtures made by
tests/golden/make_golden_hint.py from the reference HiNT_main), checkpoints, refusals, the C ABI's limits, and the restatement against
the reference's scores, window evidence and gradients."""
import ctypes
import os

import numpy as np
import pytest
import torch

from capreolus_amd import reranker
from capreolus_amd.reranker import HINT, HiNT_main
from tests import hint_case

REL = 1e-5          # of the output's scale, as in test_tk_cpu.py: the restatement repeats the reference's ATen ops (a rounding-order bound)


def _model(name):
    return hint_case.build(name, HINT)


def test_config_options_and_defaults():
    assert HINT.module_name == "HINT"
    assert HINT.config_spec == {"spatialGRU": 2, "LSTMdim": 6, "kmax": 10}
    assert HINT.supports_resident and not HINT.supports_lists
    assert "HINT" not in reranker.registry and reranker.HINT is HINT and reranker.HiNT_main is HiNT_main
    with pytest.raises(ValueError):
        HINT({"nosuchoption": 1}, hint_case.extractor("hint_small"))


@pytest.mark.parametrize("name", list(hint_case.CASES))
def test_state_dict_names_and_shapes_match_the_reference(name):
    c = hint_case.load(name)
    _, m = _model(name)
    sd = m.state_dict()
    assert sorted(sd) == [str(k) for k in c["state_keys"]]
    for k, shape in zip(c["state_keys"], c["state_shapes"]):
        assert list(sd[str(k)].shape) == [int(x) for x in shape if x], k
    assert not any("GRU2d2" in k for k in sd)
    assert not m.HiNT1.embedding.weight.requires_grad


@pytest.mark.parametrize("name", list(hint_case.CASES))
def test_fixture_ids_are_what_hint_case_draws(name):
    c = hint_case.load(name)
    ids = hint_case.inputs(name)
    np.testing.assert_array_equal(c["query"], ids[0])
    np.testing.assert_array_equal(c["posdoc"], ids[1])
    if name == "hint_grad":
        np.testing.assert_array_equal(c["negdoc"], ids[2])
    hint_case.check_ids(ids[0], ids[1])
    emb = hint_case.embeddings(name)
    assert not emb[0].any() and 0.5e-7 < np.linalg.norm(emb[hint_case.TINY_TOKEN]) < 2e-7


def test_save_and_load_weights_round_trip(tmp_path):
    r, m = _model("hint_small")
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    fn = os.path.join(tmp_path, "w", "weights")
    r.save_weights(fn, opt)
    import pickle

    with open(fn, "rb") as f:
        assert "HiNT1.embedding.weight" not in pickle.load(f)
    r2 = HINT(hint_case.config("hint_small"), hint_case.extractor("hint_small"))
    m2 = r2.build_model()
    for p in m2.parameters():
        if p.requires_grad:
            p.data.zero_()
    r2.load_weights(fn, torch.optim.Adam([p for p in m2.parameters() if p.requires_grad], lr=1e-3))
    a, b = m.state_dict(), m2.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_what_the_reference_cannot_run_is_refused():
    ex = hint_case.extractor("hint_small")
    for cfg in ({"spatialGRU": 3}, {"LSTMdim": 4}, {"kmax": 5}, {"kmax": 0}):      # (kmax 5 > 2 P = 4 at maxdoclen 200)
        with pytest.raises(ValueError):
            HINT(cfg, ex).build_model()
    # kmax > 2P at the call: a model built for longer documents, handed short ones
    ex.config = {}
    m = HINT({"kmax": 5}, ex).build_model()
    q, d = hint_case.inputs("hint_small")
    with pytest.raises(ValueError):
        m._forward_aten(torch.from_numpy(d), torch.from_numpy(q))
    with pytest.raises(ValueError):
        m._forward_aten(torch.from_numpy(d[:, :99]), torch.from_numpy(q))
    ex.embeddings = np.zeros((10, 520), dtype=np.float32)
    with pytest.raises(ValueError):
        HINT({}, ex).build_model()


def test_abi_refuses_each_geometry_limit():
    """capamd_hint_workspace_bytes / capamd_hint_forward answer -1 / CAPAMD_ERR_ARG to what the kernels do not take (no device access)"""
    from capreolus_amd import _lib

    lib = _lib.load()
    P = 0x10000
    pointers = [n for n, t in _lib.HintModel._fields_ if t is ctypes.c_void_p]

    def model(**kw):
        m = _lib.HintModel()
        for n in pointers:
            setattr(m, n, P)
        m.vocab, m.dim, m.kmax = 1000, 300, 10
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert lib.capamd_hint_workspace_bytes(ctypes.byref(model()), 4, 4, 800) > 0
    assert lib.capamd_hint_workspace_bytes(ctypes.byref(model(kmax=32)), 1, 32, 6499) > 0
    bad = [({"dim": 513}, {}), ({"dim": 0}, {}), ({"vocab": 0}, {}), ({"kmax": 0}, {}), ({"kmax": 17}, {}), ({"kmax": 33}, {"L": 6400}),
           ({"kmax": 3}, {"L": 199}), ({}, {"Q": 33}), ({}, {"Q": 0}), ({}, {"L": 99}), ({}, {"L": 6500}), ({}, {"nb": 0})]
    for mkw, skw in bad:
        m = model(**mkw)
        Q, L, nb = skw.get("Q", 4), skw.get("L", 800), skw.get("nb", 4)
        assert lib.capamd_hint_workspace_bytes(ctypes.byref(m), nb, Q, L) == -1, (mkw, skw)
        assert lib.capamd_hint_forward(P, P, 8, Q, L, ctypes.byref(m), nb, P, 1 << 40, P, None, P, None) == _lib.ERR_ARG, (mkw, skw)
    assert lib.capamd_hint_workspace_bytes(None, 4, 4, 800) == -1
    # null pointers: every argument but the optional evidence buffer and the stream, and every tensor of the model
    ok = [P, P, 8, 4, 800, None, 4, P, 1 << 40, P, None, P, None]
    for i in (0, 1, 5, 7, 9, 11):
        args = list(ok)
        args[5] = ctypes.byref(model())
        args[i] = None
        assert lib.capamd_hint_forward(*args) == _lib.ERR_ARG, i
    for n in pointers:
        assert lib.capamd_hint_forward(P, P, 8, 4, 800, ctypes.byref(model(**{n: None})), 4, P, 1 << 40, P, None, P, None) == _lib.ERR_ARG, n
    assert lib.capamd_hint_forward(P, P, -1, 4, 800, ctypes.byref(model()), 4, P, 1 << 40, P, None, P, None) == _lib.ERR_ARG
    # an empty call is fine; a short or misaligned workspace is named as such, before anything is launched
    assert lib.capamd_hint_forward(P, P, 0, 4, 800, ctypes.byref(model()), 4, P, 1 << 40, P, None, P, None) == _lib.OK
    assert lib.capamd_hint_forward(P, P, 8, 4, 800, ctypes.byref(model()), 4, P, 1000, P, None, P, None) == _lib.ERR_WORKSPACE
    assert lib.capamd_hint_forward(P, P, 8, 4, 800, ctypes.byref(model()), 4, P + 16, 1 << 40, P, None, P, None) == _lib.ERR_ALIGN


def _restated(name, dtype=torch.float32):
    c = hint_case.load(name)
    _, m = _model(name)
    m.eval()
    with torch.no_grad():
        score, ev = m._forward_aten(torch.from_numpy(c["posdoc"]), torch.from_numpy(c["query"]), dtype=dtype, return_evidence=True)
    return c, score.numpy(), ev.numpy()


@pytest.mark.parametrize("name", hint_case.SCORE_CASES)
def test_restatement_matches_the_reference(name):
    c, score, ev = _restated(name)
    want = c["evidence"].transpose(1, 0, 2)                 # the LSTM's input is [P, B, 8]
    assert ev.shape == want.shape and score.dtype == np.float32
    assert np.abs(ev - want).max() <= REL * np.abs(want).max(), np.abs(ev - want).max()
    np.testing.assert_allclose(score, c["score"], rtol=REL, atol=REL * np.abs(c["score"]).max())
    assert np.all(np.isfinite(score))


@pytest.mark.parametrize("name", hint_case.SCORE_CASES)
def test_float64_restatement_is_within_fp32_error_of_the_reference(name):
    """the reference's own fp32 error, the yardstick of the device tests: small, and not zero"""
    c, score, ev = _restated(name, torch.float64)
    assert score.dtype == np.float64
    e = np.abs(score - c["score"]).max() / np.abs(c["score"]).max()
    assert 0 < e <= REL, e


@pytest.mark.parametrize("Q,L", hint_case.SWEEP)
def test_sweep_fixture_is_the_reference_on_what_hint_case_draws(Q, L):
    """tests/golden/hint_sweep.npz (the yardstick of the device tests' sweep) belongs to hint_case.sweep_case's ids and weights"""
    cfg, ex, w, q, d = hint_case.sweep_case(Q, L)
    assert (q[1, Q - 1] == 0) and (d[1, L // 2:] == 0).all() and (d[2] == 0).all() and cfg["kmax"] <= 2 * (L // 100)
    z = hint_case.load("hint_sweep")
    m = hint_case.build_from(cfg, ex, w, HINT)[1].eval()
    with torch.no_grad():
        score, ev = m._forward_aten(torch.from_numpy(d), torch.from_numpy(q), return_evidence=True)
    want = z[f"evidence.{Q}.{L}"].transpose(1, 0, 2)
    assert np.abs(ev.numpy() - want).max() <= REL * np.abs(want).max()
    np.testing.assert_allclose(score.numpy(), z[f"score.{Q}.{L}"], rtol=REL, atol=REL * np.abs(z[f"score.{Q}.{L}"]).max())


def test_restatement_gradients_match_the_reference():
    c = hint_case.load("hint_grad")
    r, m = _model("hint_grad")
    m.train()
    b = {k: torch.from_numpy(c[k]) for k in ("query", "posdoc", "negdoc")}
    b["query_idf"] = torch.zeros(c["query"].shape)
    pos, neg = r.score(b)
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().numpy(), c["score"], rtol=REL, atol=REL * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"])).sum().backward()
    names = [k[len("grad."):] for k in c if k.startswith("grad.")]
    assert set(names) == {k for k, p in m.named_parameters() if p.requires_grad}
    params = dict(m.named_parameters())
    for k in names:
        want, got = c["grad." + k], params[k].grad.numpy()
        assert np.abs(got - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6), (k, np.abs(got - want).max(), np.abs(want).max())


def test_a_batch_equals_its_documents_one_by_one():
    c = hint_case.load("hint_small")
    _, m = _model("hint_small")
    m.eval()
    q, d = torch.from_numpy(c["query"]), torch.from_numpy(c["posdoc"])
    with torch.no_grad():
        whole = m._forward_aten(d, q)
        single = torch.cat([m._forward_aten(d[i:i + 1], q[i:i + 1]) for i in range(q.shape[0])])
    np.testing.assert_allclose(single.numpy(), whole.numpy(), rtol=REL, atol=REL * float(whole.abs().max()))


def test_scoring_without_a_device_is_an_error_not_a_fallback():
    c = hint_case.load("hint_one")
    r, m = _model("hint_one")
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        r.test({"query": torch.from_numpy(c["query"]), "posdoc": torch.from_numpy(c["posdoc"]), "query_idf": torch.zeros(c["query"].shape)})
