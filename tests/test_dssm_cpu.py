"""DSSM (reranker `DSSM`) without a GPU: the module tree and checkpoints against the reference's fixtures (tests/golden/dssm_*.npz), the
training restatement against their scores, tower outputs and gradients, the bag plumbing (capreolus_amd.bags), the refused
configurations, and the argument checks of capamd_dssm_tower (which return before anything is launched)."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from capreolus_amd import _lib, bags
from capreolus_amd.reranker import DSSM, registry
from tests import dssm_case


@pytest.mark.parametrize("name", list(dssm_case.CASES))
def test_state_dict_names_and_shapes_are_the_references(name):
    c = dssm_case.load(name)
    sd = dssm_case.build(name, DSSM)[1].state_dict()
    assert sorted(sd) == list(c["state_keys"])
    for k, shape in zip(c["state_keys"], c["state_shapes"]):
        assert list(sd[k].shape) == [int(s) for s in shape[: sd[k].dim()]], k
    n = len(dssm_case.config(name)["nhiddens"].split())
    assert set(sd) == {f"ffw.linear{i}.{k}" for i in range(n) for k in ("weight", "bias")}


def test_defaults_and_registry():
    assert DSSM.config_spec == {"nhiddens": "56"}
    assert "DSSM" not in registry and DSSM not in registry.values()
    assert not DSSM.supports_resident and not DSSM.supports_lists


def test_checkpoints_round_trip_and_load_a_reference_shaped_pickle(tmp_path):
    r, m = dssm_case.build("dssm_two", DSSM)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    fn = os.path.join(tmp_path, "w", "dssm.p")
    r.save_weights(fn, opt)
    r2, m2 = dssm_case.build_from(dssm_case.config("dssm_two"), dssm_case.extractor("dssm_two"),
                                  dssm_case.make_weights(np.random.RandomState(5), 500, "30 17"), DSSM)
    r2.load_weights(fn, torch.optim.Adam(m2.parameters(), lr=1e-4))
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k
    ref = {k: torch.from_numpy(v) for k, v in dssm_case.make_weights(np.random.RandomState(6), 500, "30 17").items()}
    fn2 = os.path.join(tmp_path, "ref.p")
    pickle.dump(ref, open(fn2, "wb"), protocol=-1)
    pickle.dump(opt.state_dict(), open(fn2 + ".optimizer", "wb"), protocol=-1)
    r2.load_weights(fn2, torch.optim.Adam(m2.parameters(), lr=1e-4))
    for k, v in ref.items():
        assert torch.equal(m2.state_dict()[k], v), k


@pytest.mark.parametrize("name", dssm_case.SCORE_CASES)
def test_restatement_equals_the_reference_from_bags_and_from_dense(name):
    c = dssm_case.load(name)
    m = dssm_case.build(name, DSSM)[1].eval()
    q, d = dssm_case.bags_of(c, "query"), dssm_case.bags_of(c, "posdoc")
    with torch.no_grad():
        s, qt, dt = m._forward_aten(d, q, return_towers=True)
        s2 = m._forward_aten(d.to_dense(m.nvocab), q.to_dense(m.nvocab))
    assert torch.equal(s, s2)
    np.testing.assert_allclose(s.numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    np.testing.assert_allclose(qt.numpy(), c["qtower"], rtol=1e-5, atol=1e-5 * np.abs(c["qtower"]).max())
    np.testing.assert_allclose(dt.numpy(), c["dtower"], rtol=1e-5, atol=1e-5 * np.abs(c["dtower"]).max())


def test_gradients_equal_the_reference():
    c = dssm_case.load("dssm_grad")
    r, m = dssm_case.build("dssm_grad", DSSM)
    m.train()
    for mod in m.ffw:
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0                                     # (the fixture's gradients are those of the function itself)
    batch = {k: dssm_case.bags_of(c, k).to_dense(m.nvocab) for k in ("query", "posdoc", "negdoc")}
    batch["query_idf"] = torch.zeros(6, 4)
    pos, neg = r.score(batch)
    assert pos.requires_grad and neg.requires_grad
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"])).sum().backward()
    for k, p in m.named_parameters():
        want = c["grad." + k]
        assert np.abs(want).max() > 0 and np.abs(p.grad.numpy() - want).max() <= 1e-4 * np.abs(want).max(), k


def test_dropout_is_live_in_training_mode_only():
    c = dssm_case.load("dssm_grad")
    m = dssm_case.build("dssm_grad", DSSM)[1]
    q, d = dssm_case.bags_of(c, "query"), dssm_case.bags_of(c, "posdoc")
    m.train()
    torch.manual_seed(0)
    a = m._forward_aten(d, q)
    b = m._forward_aten(d, q)
    assert not torch.equal(a, b)
    m.eval()
    assert torch.equal(m._forward_aten(d, q), m._forward_aten(d, q))


@pytest.mark.parametrize("name", list(dssm_case.CASES))
def test_from_dense_equals_from_term_ids_on_the_fixture_documents(name):
    c = dssm_case.load(name)
    nvocab = int(c["nvocab"])
    for side, rows in zip(("query", "posdoc"), dssm_case.rows(name)):
        b = bags.from_term_ids(rows)
        assert b.indptr.dtype == torch.int64 and b.idx.dtype == torch.int32 and b.val.dtype == torch.float32
        got = bags.from_dense(b.to_dense(nvocab))
        for x, y in zip(got, b):
            assert torch.equal(x, y) and x.dtype == y.dtype
        fix = dssm_case.bags_of(c, side)
        assert torch.equal(fix.indptr, b.indptr) and torch.equal(fix.idx, b.idx)
        if not dssm_case.CASES[name].get("fractional"):
            assert torch.equal(fix.val, b.val)
        for n in range(b.rows):                             # entries ordered by index inside every bag
            seg = b.idx[b.indptr[n]:b.indptr[n + 1]]
            assert (seg[1:] > seg[:-1]).all()
    assert bags.from_term_ids([]).rows == 0 and bags.from_term_ids([[], [3, 3]]).val.tolist() == [2.0]
    with pytest.raises(ValueError):
        bags.from_dense(torch.zeros(4))


@pytest.mark.parametrize("nhiddens,nvocab,word", [("", 10, "layers"), ("5 5 5 5 5", 10, "layers"), ("513", 10, "widths"), ("56 0", 10, "widths"),
                                                  ("56 x", 10, "nhiddens"), ("56", 0, "vocabulary")])
def test_refused_configurations_raise(nhiddens, nvocab, word):
    with pytest.raises(ValueError, match=word):
        DSSM({"nhiddens": nhiddens}, dssm_case.make_extractor(nvocab)).build_model()


def test_engine_refuses_host_tensors():
    c = dssm_case.load("dssm_default")
    r, m = dssm_case.build("dssm_default", DSSM)
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        r.test({"query": dssm_case.bags_of(c, "query"), "posdoc": dssm_case.bags_of(c, "posdoc"), "query_idf": None})


P = 1 << 20       # a well aligned address that is never dereferenced: every call below returns before a launch


def _model(layers=2, widths=(56, 17, 0, 0), nvocab=500, w1t=P, b1=P, w=(P, 0, 0), b=(P, 0, 0)):
    m = _lib.DssmModel()
    m.w1t, m.b1, m.nvocab, m.layers = w1t, b1, nvocab, layers
    for i in range(4):
        m.width[i] = widths[i]
    for i in range(3):
        m.w[i], m.b[i] = w[i] or None, b[i] or None
    return m


def _tower(m, indptr=P, idx=P, val=P, N=3, nnz=9, side=1, rep=P, status=P):
    vp = lambda a: ctypes.c_void_p(a) if a else None       # noqa: E731
    return _lib.load().capamd_dssm_tower(vp(indptr), vp(idx), vp(val), N, nnz, ctypes.byref(m) if m is not None else None, side, vp(rep), vp(status), None)


def test_tower_entry_refuses_null_pointers_and_every_limit():
    for k in ("indptr", "idx", "val", "rep", "status"):
        assert _tower(_model(), **{k: 0}) == _lib.ERR_ARG, k
    assert _tower(None) == _lib.ERR_ARG
    for kw in (dict(layers=0), dict(layers=5), dict(widths=(0, 17, 0, 0)), dict(widths=(513, 17, 0, 0)), dict(widths=(56, 513, 0, 0)), dict(nvocab=0),
               dict(nvocab=1 << 31), dict(w1t=0), dict(b1=0), dict(w=(0, 0, 0)), dict(b=(0, 0, 0))):
        assert _tower(_model(**kw)) == _lib.ERR_ARG, kw
    for kw in (dict(N=-1), dict(N=1 << 31), dict(nnz=-1), dict(side=2)):
        assert _tower(_model(), **kw) == _lib.ERR_ARG, kw
    assert _tower(_model(w1t=P + 4)) == _lib.ERR_ALIGN
    assert _tower(_model(), indptr=P + 4) == _lib.ERR_ALIGN
    assert _tower(_model(), N=0) == _lib.OK                                        # nothing to do, nothing launched
    assert _tower(_model(), N=0, nnz=0, idx=0, val=0) == _lib.OK                   # no entries: idx / val may be null
