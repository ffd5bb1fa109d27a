"""DUET (reranker `DUET`) without a GPU: the module tree against the reference's fixtures (tests/golden/duet_*.npz), the torch
restatement (what training and the CPU run) and the numpy float64 restatement against their scores, parts, query vectors, pooled maps and
gradients, the refused geometries, a batch of one, and the argument checks of capamd_duet_forward / capamd_duet_workspace_bytes (which
return before anything is launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from capreolus_amd import _lib
from capreolus_amd.reranker import DUET, registry
from tests import duet_case


def _aten(m, q, d, idf, dtype=torch.float32):
    with torch.no_grad():
        out = m._forward_aten(torch.from_numpy(d), torch.from_numpy(q), torch.from_numpy(idf), dtype=dtype, return_parts=True)
    return dict(zip(duet_case.OUTPUTS, (t.numpy() for t in out)))


@pytest.mark.parametrize("name", list(duet_case.CASES))
def test_state_dict_names_and_shapes_are_the_references(name):
    c = duet_case.load(name)
    sd = duet_case.build(name, DUET)[1].state_dict()
    assert sorted(sd) == list(c["state_keys"])
    for k, shape in zip(c["state_keys"], c["state_shapes"]):
        assert list(sd[k].shape) == [int(s) for s in shape[: sd[k].dim()]], k
    assert len(sd) == 19 and "dm.embedding.weight" in sd and "lm.ffw.3.weight" in sd and "dm.ffw_2.1.bias" in sd


def test_defaults_and_registry():
    assert DUET.config_spec == {"nfilters": 10, "lmhidden": 30, "nhidden": 699, "idfweight": True, "dropoutrate": 0.5, "activation": "relu"}
    assert DUET.module_name == "DUET" and "DUET" not in registry and DUET not in registry.values()


@pytest.mark.parametrize("name", duet_case.SCORE_CASES)
def test_restatements_equal_the_reference(name):
    c = duet_case.load(name)
    duet_case.check_ids(c["query"], c["posdoc"], c["query_idf"])
    m = duet_case.build(name, DUET)[1].eval()
    got = _aten(m, c["query"], c["posdoc"], c["query_idf"])
    f64 = duet_case.restate(duet_case.config(name), duet_case.embeddings(name), duet_case.weights(name), c["query"], c["posdoc"], c["query_idf"])
    t64 = _aten(m, c["query"], c["posdoc"], c["query_idf"], dtype=torch.float64)
    for k in duet_case.OUTPUTS:
        scale = max(np.abs(c[k]).max(), 1e-30)
        np.testing.assert_allclose(got[k], c[k], rtol=1e-5, atol=1e-5 * scale, err_msg=k)
        np.testing.assert_allclose(f64[k], c[k], rtol=1e-5, atol=1e-5 * scale, err_msg=k)
        np.testing.assert_allclose(t64[k], f64[k], rtol=1e-12, atol=1e-12 * scale, err_msg=k)         # the two float64 restatements agree


def test_a_pad_in_the_query_matches_every_pad_in_the_document():
    """pair 1 of a fixture: a padded tail under a query whose last term is a pad with idf > 0.  The reference's local score moves with that
    idf (the fixture has it); with the idf at 0 the pads' columns drop out"""
    c = duet_case.load("duet_default")
    cfg, emb, w = duet_case.config("duet_default"), duet_case.embeddings("duet_default"), duet_case.weights("duet_default")
    idf0 = c["query_idf"].copy()
    idf0[1, 3] = 0.0
    with_pads = duet_case.restate(cfg, emb, w, c["query"], c["posdoc"], c["query_idf"])["lm"]
    without = duet_case.restate(cfg, emb, w, c["query"], c["posdoc"], idf0)["lm"]
    assert abs(with_pads[1] - without[1]) > 1e-2 and abs(c["lm"][1] - with_pads[1]) < 1e-4 * abs(with_pads[1])
    assert np.array_equal(np.delete(with_pads, 1), np.delete(without, 1))


def test_gradients_equal_the_reference():
    c = duet_case.load("duet_grad")
    r, m = duet_case.build("duet_grad", DUET)
    m.train()
    pos, neg = r.score({"query": torch.from_numpy(c["query"]), "posdoc": torch.from_numpy(c["posdoc"]), "negdoc": torch.from_numpy(c["negdoc"]),
                        "query_idf": torch.from_numpy(c["query_idf"])})
    assert pos.requires_grad and neg.requires_grad and pos.shape == neg.shape == (c["query"].shape[0],)
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"])).sum().backward()
    params = dict(m.named_parameters())
    names = [k[5:] for k in c if k.startswith("grad.")]
    assert sorted(names) == sorted(k for k, p in params.items() if p.requires_grad) and len(names) == 18
    for k in names:
        g, want = params[k].grad.numpy(), c["grad." + k]
        assert g.shape == want.shape and np.abs(want).max() > 0 and np.abs(g - want).max() <= 1e-4 * np.abs(want).max(), k


def test_a_batch_of_one_works_and_equals_its_row_of_the_batch():
    c = duet_case.load("duet_min")
    r, m = duet_case.build("duet_min", DUET)
    m.eval()
    with torch.no_grad():
        for i in range(c["query"].shape[0]):
            one = r.test({"query": torch.from_numpy(c["query"][i:i + 1]), "posdoc": torch.from_numpy(c["posdoc"][i:i + 1]),
                          "query_idf": torch.from_numpy(c["query_idf"][i:i + 1])})
            assert one.shape == (1,)
            np.testing.assert_allclose(one.numpy(), c["score"][i:i + 1], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())


@pytest.mark.parametrize("maxqlen,maxdoclen,cfg,word", [(3, 230, {"nhidden": 129}, "maxqlen"), (5, 230, {"nhidden": 129}, "maxqlen"),
                                                        (4, 230, {"nhidden": 129, "nfilters": 1}, "nfilters"), (4, 102, {"nhidden": 1}, "maxdoclen"),
                                                        (4, 230, {"nhidden": 699}, "nhidden"), (4, 800, {"nhidden": 700}, "nhidden")])
def test_refused_geometries_name_their_condition(maxqlen, maxdoclen, cfg, word):
    from types import SimpleNamespace

    ex = SimpleNamespace(embeddings=np.zeros((8, 24), dtype=np.float32), config={"maxqlen": maxqlen, "maxdoclen": maxdoclen})
    with pytest.raises(ValueError, match=word):
        DUET(cfg, ex).build_model()


@pytest.mark.parametrize("cfg,dim,maxdoclen,word", [({"nfilters": 33}, 24, 800, "nfilters"), ({"lmhidden": 257}, 24, 800, "lmhidden"),
                                                    ({"lmhidden": 0}, 24, 800, "lmhidden"), ({}, 513, 800, "dim"),
                                                    ({"nhidden": 8092}, 24, 8193, "maxdoclen"), ({"activation": "gelu"}, 24, 800, "activation")])
def test_configurations_beyond_the_kernels_limits_raise(cfg, dim, maxdoclen, word):
    from types import SimpleNamespace

    ex = SimpleNamespace(embeddings=np.zeros((8, dim), dtype=np.float32), config={"maxqlen": 4, "maxdoclen": maxdoclen})
    with pytest.raises(ValueError, match=word):
        DUET(cfg, ex).build_model()


def test_documents_of_another_length_than_the_models_raise():
    r, m = duet_case.build("duet_min", DUET)
    m.eval()
    with torch.no_grad(), pytest.raises(ValueError, match="nhidden|maxdoclen"):
        r.test({"query": torch.ones(2, 4, dtype=torch.int64), "posdoc": torch.ones(2, 104, dtype=torch.int64), "query_idf": torch.ones(2, 4)})


def test_header_and_binding_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "capreolus_amd.h")).read()
    assert int(re.search(r"#define CAPAMD_VERSION (\d+)", hdr).group(1)) == _lib.VERSION == 405
    for name in ("capamd_duet_forward", "capamd_duet_workspace_bytes"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr)
    # the struct's fields, in the header's order, are the binding's
    body = re.search(r"typedef struct capamd_duet_model \{(.*?)\} capamd_duet_model;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip(" *") for n in re.sub(r"^(const float|int64_t|int)\s*", "", decl).split(",")]
    assert fields == [n for n, _ in _lib.DuetModel._fields_]
    assert len(_lib.SIGNATURES["capamd_duet_forward"][1]) == 15 and len(_lib.SIGNATURES["capamd_duet_workspace_bytes"][1]) == 4


P = ctypes.c_void_p(1 << 20)       # a well aligned address that is never dereferenced: every call below returns before a launch


def _model(**kw):
    m = _lib.DuetModel()
    for n, t in _lib.DuetModel._fields_:
        if t is ctypes.c_void_p:
            setattr(m, n, 1 << 20)
    m.vocab, m.dim, m.nfilters, m.lmhidden, m.maxdoclen, m.nhidden, m.activation, m.idfweight = 64, 24, 10, 30, 800, 699, 0, 1
    for k, v in kw.items():
        setattr(m, k, v)
    return m


REFUSED = (dict(Q=3), dict(Q=5), dict(nfilters=1), dict(nfilters=33), dict(L=102, maxdoclen=102, nhidden=1), dict(L=8193, maxdoclen=8193, nhidden=8092),
           dict(nhidden=700), dict(maxdoclen=801), dict(lmhidden=0), dict(lmhidden=257), dict(dim=0), dict(dim=513), dict(vocab=0), dict(activation=2))


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_entry_and_workspace_query_refuse_geometry(kw):
    lib = _lib.load()
    kw = dict(kw)
    Q, L = kw.pop("Q", 4), kw.pop("L", 800)
    m = _model(**kw)
    assert lib.capamd_duet_workspace_bytes(ctypes.byref(m), 4, Q, L) == -1
    assert lib.capamd_duet_forward(P, P, P, 3, Q, L, ctypes.byref(m), 4, P, 1 << 30, P, None, None, P, None) == _lib.ERR_ARG


def test_entry_refuses_null_pointers_and_small_workspaces():
    lib = _lib.load()
    m = _model()
    need = lib.capamd_duet_workspace_bytes(ctypes.byref(m), 4, 4, 800)
    assert need == 4 * 800 * 32 * 4                                                # 3 H = 30 projections per term, held as 32
    assert lib.capamd_duet_workspace_bytes(ctypes.byref(m), 0, 4, 800) == -1

    def call(q=P, d=P, idf=P, B=3, model=m, nb=4, ws=P, ws_bytes=need, out=P, status=P):
        return lib.capamd_duet_forward(q, d, idf, B, 4, 800, ctypes.byref(model), nb, ws, ws_bytes, out, None, None, status, None)

    for k in ("q", "d", "idf", "ws", "out", "status"):
        assert call(**{k: None}) == _lib.ERR_ARG, k
    assert call(idf=None, model=_model(idfweight=0), B=0) == _lib.OK               # without idfweight no idf is read
    for n, t in _lib.DuetModel._fields_:
        if t is ctypes.c_void_p:
            assert call(model=_model(**{n: None})) == _lib.ERR_ARG, n
    assert call(B=-1) == _lib.ERR_ARG and call(nb=0) == _lib.ERR_ARG
    assert call(model=_model(emb=(1 << 20) + 4)) == _lib.ERR_ALIGN
    assert call(ws_bytes=3 * 800 * 32 * 4 - 1) == _lib.ERR_WORKSPACE               # three documents in one micro-batch
    assert call(ws=ctypes.c_void_p((1 << 20) + 64)) == _lib.ERR_ALIGN
    assert call(B=0) == _lib.OK                                                    # nothing to do, nothing launched
