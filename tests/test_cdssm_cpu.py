"""CDSSM (reranker `CDSSM`) without a GPU: the module tree and checkpoints against the reference's fixtures (tests/golden/cdssm_*.npz),
the training restatement against their scores, tower outputs and gradients, the refused configurations, and the argument checks of
capamd_cdssm_tower / capamd_cos_sigmoid_pairs (which return before anything is launched)."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

from capreolus_amd import _lib
from capreolus_amd.reranker import CDSSM, registry
from tests import cdssm_case


@pytest.mark.parametrize("name", list(cdssm_case.CASES))
def test_state_dict_names_and_shapes_are_the_references(name):
    c = cdssm_case.load(name)
    sd = cdssm_case.build(name, CDSSM)[1].state_dict()
    assert sorted(sd) == list(c["state_keys"])
    for k, shape in zip(c["state_keys"], c["state_shapes"]):
        assert list(sd[k].shape) == [int(s) for s in shape[: sd[k].dim()]], k
    assert {"embedding.weight", "conv.0.weight", "conv.0.bias", "ffw.weight", "ffw.bias"} == set(sd)


def test_defaults_and_registry():
    assert CDSSM.config_spec == {"nkernel": 3, "nfilter": 1, "nhiddens": 30, "windowsize": 3, "dropoutrate": 0}
    assert "CDSSM" not in registry and CDSSM not in registry.values()
    assert CDSSM.supports_resident and not CDSSM.supports_lists


def test_checkpoints_round_trip_and_load_a_reference_shaped_pickle(tmp_path):
    r, m = cdssm_case.build("cdssm_multiple", CDSSM)
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    fn = os.path.join(tmp_path, "w", "cdssm.p")
    r.save_weights(fn, opt)
    saved = pickle.load(open(fn, "rb"))
    assert sorted(saved) == ["conv.0.bias", "conv.0.weight", "ffw.bias", "ffw.weight"]          # the frozen table is never written
    r2, m2 = cdssm_case.build_from(cdssm_case.config("cdssm_multiple"), cdssm_case.extractor("cdssm_multiple"),
                                   cdssm_case.make_weights(np.random.RandomState(5), cdssm_case.config("cdssm_multiple")), CDSSM)
    r2.load_weights(fn, torch.optim.Adam([p for p in m2.parameters() if p.requires_grad], lr=1e-3))
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k
    # what the reference writes: a plain pickled state_dict without the table
    ref = {k: torch.from_numpy(v) for k, v in cdssm_case.weights("cdssm_multiple").items()}
    fn2 = os.path.join(tmp_path, "ref.p")
    pickle.dump(ref, open(fn2, "wb"), protocol=-1)
    pickle.dump(opt.state_dict(), open(fn2 + ".optimizer", "wb"), protocol=-1)
    r2.load_weights(fn2, torch.optim.Adam([p for p in m2.parameters() if p.requires_grad], lr=1e-3))
    for k, v in ref.items():
        assert torch.equal(m2.state_dict()[k], v), k


@pytest.mark.parametrize("name", cdssm_case.SCORE_CASES)
def test_restatement_equals_the_reference(name):
    c = cdssm_case.load(name)
    m = cdssm_case.build(name, CDSSM)[1].eval()
    with torch.no_grad():
        s, q, d = m._forward_aten(torch.from_numpy(c["posdoc"]), torch.from_numpy(c["query"]), return_towers=True)
    np.testing.assert_allclose(s.numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    np.testing.assert_allclose(q.numpy(), c["qtower"], rtol=1e-5, atol=1e-5 * max(np.abs(c["qtower"]).max(), 1e-30))
    np.testing.assert_allclose(d.numpy(), c["dtower"], rtol=1e-5, atol=1e-5 * max(np.abs(c["dtower"]).max(), 1e-30))
    if name == "cdssm_negbias":
        assert s[-1].item() == 0.5 and c["score"][-1] == 0.5 and not d[-1].any()


def test_engine_refuses_host_tensors():
    c = cdssm_case.load("cdssm_one")
    r, m = cdssm_case.build("cdssm_one", CDSSM)
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        r.test({"query": torch.from_numpy(c["query"]), "posdoc": torch.from_numpy(c["posdoc"])})


def test_gradients_equal_the_reference():
    c = cdssm_case.load("cdssm_grad")
    r, m = cdssm_case.build("cdssm_grad", CDSSM)
    m.train()
    pos, neg = r.score({"query": torch.from_numpy(c["query"]), "posdoc": torch.from_numpy(c["posdoc"]), "negdoc": torch.from_numpy(c["negdoc"])})
    assert pos.requires_grad and neg.requires_grad
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"])).sum().backward()
    params = dict(m.named_parameters())
    for k in ("conv.0.weight", "conv.0.bias"):
        g, want = params[k].grad.numpy(), c["grad." + k]
        assert np.abs(want).max() > 0 and np.abs(g - want).max() <= 1e-4 * np.abs(want).max(), k
    assert params["ffw.weight"].grad is None and "grad.ffw.weight" not in c                      # in the state_dict, never used


@pytest.mark.parametrize("cfg,dim,word", [({"windowsize": 9}, 24, "windowsize"), ({"windowsize": 0}, 24, "windowsize"), ({"windowsize": 8}, 513, "dim"),
                                          ({"windowsize": 1}, 600, "dim"), ({"nkernel": 17}, 24, "nkernel"), ({"nkernel": 0}, 24, "nkernel"),
                                          ({"windowsize": 1, "nkernel": 5}, 4, "nkernel"), ({"nfilter": 17}, 24, "nfilter"), ({"nfilter": 0}, 24, "nfilter")])
def test_refused_configurations_raise(cfg, dim, word):
    from types import SimpleNamespace

    ex = SimpleNamespace(embeddings=np.zeros((8, dim), dtype=np.float32))
    with pytest.raises(ValueError, match=word):
        CDSSM(cfg, ex).build_model()


def test_header_and_binding_agree_on_the_new_status_bit_and_the_version():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "capreolus_amd.h")).read()
    assert int(re.search(r"#define CAPAMD_STATUS_BAG_RANGE (\d+)", hdr).group(1)) == _lib.STATUS_BAG_RANGE == 256
    assert int(re.search(r"#define CAPAMD_VERSION (\d+)", hdr).group(1)) == _lib.VERSION == 405
    for name in ("capamd_cdssm_tower", "capamd_dssm_tower", "capamd_cos_sigmoid_pairs"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr)


P = ctypes.c_void_p(1 << 20)       # a well aligned address that is never dereferenced: every call below returns before a launch


def _tower(ids=P, N=3, T=5, emb=P, vocab=64, dim=24, W=3, w=P, b=P, nk=3, F=1, side=1, rep=P, status=P):
    return _lib.load().capamd_cdssm_tower(ids, N, T, emb, vocab, dim, W, w, b, nk, F, side, rep, status, None)


def test_tower_entry_refuses_null_pointers_and_every_limit():
    for k in ("ids", "emb", "w", "b", "rep", "status"):
        assert _tower(**{k: None}) == _lib.ERR_ARG, k
    for kw in (dict(dim=0), dict(dim=513), dict(W=0), dict(W=9), dict(W=8, dim=516), dict(nk=0), dict(nk=17), dict(W=1, dim=4, nk=5), dict(F=0), dict(F=17),
               dict(T=0), dict(N=-1), dict(N=1 << 31), dict(vocab=0), dict(side=2)):
        assert _tower(**kw) == _lib.ERR_ARG, kw
    assert _tower(emb=ctypes.c_void_p((1 << 20) + 4)) == _lib.ERR_ALIGN
    assert _tower(ids=ctypes.c_void_p((1 << 20) + 4)) == _lib.ERR_ALIGN
    assert _tower(N=0) == _lib.OK                                                  # nothing to do, nothing launched


def test_pair_entry_refuses_null_pointers_and_bad_sizes():
    def pairs(q=P, d=P, pq=P, pd=P, Nq=2, Nd=5, n=5, R=7, out=P, status=P):
        return _lib.load().capamd_cos_sigmoid_pairs(q, d, pq, pd, Nq, Nd, n, R, out, status, None)

    for k in ("q", "d", "out", "status"):
        assert pairs(**{k: None}) == _lib.ERR_ARG, k
    for kw in (dict(Nq=0), dict(Nd=0), dict(n=-1), dict(R=0), dict(pq=None), dict(pd=None, n=6)):     # (no index array: pair i is row i)
        assert pairs(**kw) == _lib.ERR_ARG, kw
    assert pairs(pq=ctypes.c_void_p((1 << 20) + 2)) == _lib.ERR_ALIGN
    assert pairs(n=0) == _lib.OK
