"""Birch (reranker `birch`) on the host: the float64 restatement of what the reference does around its encoder (tests/birch_case.py)
against the fixtures made from the reference Birch_Class (tests/golden/make_golden_birch.py), the plugin's parameter surface and
refusals, and the C ABI's new entries (no device work: argument checks come first)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from capreolus_amd import _lib, engine
from capreolus_amd.reranker import Birch, Birch_Class
from tests import birch_case
from tests.birch_case import CASES, GRAD_CASES, load_birch_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = dict(hidden=64, layers=1, heads=1, ffn=128, vocab=200, max_pos=64)


def _plugin(geom, P, S, **cfg):
    return Birch(dict({"pretrained": geom}, **cfg), SimpleNamespace(config={"numpassages": P, "maxseqlen": S}))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    c, bert, combine, geom = load_birch_case(name)
    B, P, S = c["pos_bert_input"].shape
    plan = birch_case.plan_restated(c["pos_mask"], c["pos_seg"], B, "reference")
    # the sub-batches the reference's encoder saw: (rows, cut + 1) each
    df, shapes = plan["doc_first"], []
    for b in range(B):
        for r0 in range(df[b], df[b + 1], B):
            shapes.append((min(B, df[b + 1] - r0), int(plan["cut"][r0]) + 1))
    assert shapes == [tuple(int(x) for x in s) for s in c["subbatch_shapes"]]
    assert len(c["ref_enc_logits"]) == df[-1] == len(c["ref_full_logits"])
    got, top, ps = birch_case.head_restated(c["ref_enc_logits"], df, P, int(c["topk"]), combine)
    ref = c["ref_score"].astype(np.float64)
    assert np.abs(got - ref).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max()) * max(1, int(c["hidden"])), (got, ref)
    assert (np.diff(top, axis=1) <= 0).all() and ps.shape == (B, P)
    # truncate = "none" encodes the same rows, whole
    full = birch_case.plan_restated(c["pos_mask"], c["pos_seg"], 2, "none")
    assert full["rows"] == plan["rows"] and (full["cut"] == S - 1).all()
    assert np.array_equal(full["enc_mask"], np.stack([c["pos_mask"][b, p] for b, p in plan["rows"]]))


def test_fixtures_cover_what_they_are_for():
    c = load_birch_case("birch_mini")[0]
    B, P, S = c["pos_bert_input"].shape
    valid = ((c["pos_mask"].astype(int) + c["pos_seg"]) == 2).sum(-1) > 2
    assert sorted(valid.sum(1)) == [0, 1, 2, 4, P] and P % B != 0
    c = load_birch_case("birch_mixed")[0]
    B, P, S = c["pos_bert_input"].shape
    sm = c["pos_mask"].astype(int) + c["pos_seg"]
    twos = (sm == 2).sum(-1)
    assert 2 in twos and 3 in twos
    plan = birch_case.plan_restated(c["pos_mask"], c["pos_seg"], B, "reference")
    own = np.array([int(np.argmax(sm[b, p])) for b, p in plan["rows"]])
    assert (plan["cut"] > own).any()                         # a sub-batch's cut that is not the row's own
    first_pad = np.array([int(np.argmax(np.append(c["pos_bert_input"][b, p] == 0, True))) for b in range(B) for p in range(P)])
    holes = [(c["pos_mask"].reshape(B * P, S)[i, :first_pad[i]] == 0).any() for i in range(B * P)]
    assert any(holes)
    c = load_birch_case("birch_wide")[0]
    assert [int(x) for x in c["dims"][:4]] == [1024, 2, 16, 4096]


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_match_the_reference(name):
    c, bert, combine, geom = load_birch_case(name)
    r = _plugin(geom, int(c["P"]), int(c["S"]), topk=int(c["topk"]), hidden=int(c["hidden"]))
    m = r.build_model()
    sd = {k: v for k, v in m.state_dict().items() if not k.endswith("position_ids")}
    assert sorted(sd) == [str(k) for k in c["state_keys"]]
    missing = m.bert.load_state_dict(bert, strict=False)
    assert not missing.unexpected_keys and not [k for k in missing.missing_keys if "position_ids" not in k]
    assert not m.load_state_dict(combine, strict=False).unexpected_keys
    p = m._bert_params()
    assert p["classifier.weight"] is m.bert.cls.seq_relationship.weight and "bert.pooler.dense.weight" in p


@pytest.mark.parametrize("topk", [1, 3, 7])
def test_combine_starts_as_the_mean_of_the_top_k(topk):
    m = _plugin(GEOM, 8, 32, topk=topk).build_model()
    assert torch.equal(m.combine.weight, torch.ones(1, topk) / topk) and m.combine.bias is None
    assert sorted(m.combine_params()) == ["combine.weight"]
    m = _plugin(GEOM, 8, 32, topk=topk, hidden=5).build_model()
    assert sorted(m.combine_params()) == ["combine.0.bias", "combine.0.weight", "combine.2.bias", "combine.2.weight"]
    assert m.combine[0].weight.shape == (5, topk)


def test_refusals_by_name():
    with pytest.raises(ValueError, match="topk = 4 is larger than the extractor's numpassages = 3"):
        _plugin(GEOM, 3, 32, topk=4).build_model()
    with pytest.raises(ValueError, match="passages per document"):
        _plugin(GEOM, 65, 32).build_model()
    with pytest.raises(ValueError, match="hidden must lie in 0..256"):
        _plugin(GEOM, 4, 32, hidden=257).build_model()
    with pytest.raises(ValueError, match="unsupported passage length 48"):
        _plugin(GEOM, 4, 48).build_model()
    with pytest.raises(ValueError, match="truncate must be one of"):
        _plugin(GEOM, 4, 32, truncate="paper").build_model()
    with pytest.raises(ValueError, match="unknown config options"):
        _plugin(GEOM, 4, 32, aggregation="max")
    with pytest.raises(ValueError, match="subbatch must be at least 1"):
        engine.BirchEngine.check_dims(4, 32, 3, 0, subbatch=0)
    with pytest.raises(ValueError, match="truncate"):
        engine.BirchEngine(None, truncate="cut")


def test_fine_tuning_the_encoder_raises_and_cpu_tensors_are_refused():
    x = torch.zeros((2, 4, 32), dtype=torch.int64)
    m = _plugin(GEOM, 4, 32, finetune=True).build_model()
    m.train()
    with pytest.raises(NotImplementedError, match="fine-tuning the encoder"):
        m(x, x, x)
    assert m._engine is None
    m = _plugin(GEOM, 4, 32).build_model().eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x, x, x)


def test_batch_coupled_follows_truncate():
    assert _plugin(GEOM, 4, 32).batch_coupled is True and _plugin(GEOM, 4, 32).config["truncate"] == "reference"
    assert _plugin(GEOM, 4, 32, truncate="none").batch_coupled is False
    assert Birch.module_name == "birch" and Birch_Class.__name__ == "Birch_Class"
    from capreolus_amd import reranker

    assert "birch" not in reranker.registry
    assert {k: Birch.config_spec[k] for k in ("topk", "hidden", "finetune", "pretrained")} == {"topk": 3, "hidden": 0, "finetune": False,
                                                                                               "pretrained": "msmarco_mb"}


def test_header_and_binding_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "capreolus_amd.h")).read()
    assert int(re.search(r"#define CAPAMD_VERSION (\d+)", hdr).group(1)) == _lib.VERSION == 405
    lib = _lib.load()
    assert lib.capamd_version() == 405
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("capamd_birch_workspace_bytes", "capamd_birch_plan", "capamd_birch_head"):
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_entries_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    X = 0x10000          # (device pointers are never dereferenced on the host: any aligned non-null value will do)

    def plan(B=2, P=4, S=64, subbatch=2, truncate=1, ids=X, n_enc=X, ws=X, ws_bytes=1 << 20):
        return lib.capamd_birch_plan(ids, X, X, B, P, S, subbatch, truncate, ws, ws_bytes, X, X, X, X, n_enc, None)

    for kw in ({"P": 0}, {"P": 65}, {"S": 48}, {"S": 0}, {"S": 288}, {"S": 1024}, {"subbatch": 0}, {"truncate": 2}, {"truncate": -1}, {"B": -1},
               {"B": 1 << 30, "P": 64}, {"ids": None}, {"n_enc": None}, {"ws": None}):
        assert plan(**kw) == _lib.ERR_ARG, kw
    assert plan(ws_bytes=16) == _lib.ERR_WORKSPACE
    assert plan(ws=X + 16) == _lib.ERR_ALIGN

    def head(B=2, P=4, topk=3, hidden=0, n=5, w1=X, b1=None, w2=None, b2=None, out=X):
        return lib.capamd_birch_head(X, n, X, B, P, topk, hidden, w1, b1, w2, b2, out, None, None, None)

    for kw in ({"topk": 0}, {"topk": 5}, {"P": 65, "topk": 65}, {"P": 0}, {"hidden": -1}, {"hidden": 257, "b1": X, "w2": X, "b2": X}, {"hidden": 8},
               {"hidden": 8, "b1": X, "w2": X}, {"w1": None}, {"out": None}, {"B": -1}, {"n": -1}):
        assert head(**kw) == _lib.ERR_ARG, kw
    assert head(B=0) == _lib.OK and head(B=0, hidden=8, b1=X, w2=X, b2=X) == _lib.OK       # nothing to launch


def test_workspace_bytes():
    lib = _lib.load()
    up = lambda n: (4 * n + 255) // 256 * 256
    for B, P in ((1, 1), (5, 6), (67, 64), (1000, 16), (0, 3)):
        assert lib.capamd_birch_workspace_bytes(B, P) == 4 * up(B * P) + up(B), (B, P)
    for B, P in ((1, 0), (1, 65), (-1, 4), (1 << 30, 64)):
        assert lib.capamd_birch_workspace_bytes(B, P) == -1, (B, P)


@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradient_restatement_reproduces_the_reference(name):
    c, bert, combine, geom = load_birch_case(name)
    g = np.load(os.path.join(birch_case.GOLDEN, "birch_grad.npz"))
    B, P, S = c["pos_bert_input"].shape
    topk = int(c["topk"])
    df = birch_case.plan_restated(c["pos_mask"], c["pos_seg"], B, "reference")["doc_first"]
    ndf = birch_case.plan_restated(g[f"{name}.neg_mask"], g[f"{name}.neg_seg"], B, "reference")["doc_first"]
    tp = birch_case.head_restated(c["ref_enc_logits"], df, P, topk, combine)[1]
    tn = birch_case.head_restated(g[f"{name}.neg_enc_logits"], ndf, P, topk, combine)[1]
    grads, _, d = birch_case.grad_restated(tp, tn, combine)
    assert abs(np.mean(1.0 - 1.0 / (1.0 + np.exp(-d))) - float(g[f"{name}.loss"])) <= 1e-6
    for k, v in grads.items():
        ref = g[f"{name}.grad.{k}"]
        assert v.shape == ref.shape and np.abs(v - ref).max() <= 1e-6, k
    eps = birch_case.E2E_FACTOR["fp16"] * max(np.abs(c["ref_enc_logits_amp_fp16"] - c["ref_enc_logits"]).max(),
                                              np.abs(g[f"{name}.neg_enc_logits_amp_fp16"] - g[f"{name}.neg_enc_logits"]).max()) + 1e-4
    assert birch_case.relu_margin_ok(tp, tn, combine, eps)   # the premise of the GPU test's gradient bound
