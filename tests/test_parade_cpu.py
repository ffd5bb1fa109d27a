"""PARADE (reranker `ptparade`) on the host: the plugin's parameter surface against the reference's (fixtures made by
tests/golden/make_golden_parade.py from the reference PTParade_Class), its refusals, and a numpy restatement of the aggregation head
that pins what the fixtures mean."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from capreolus_amd.reranker import PTParade, PTParade_Class
from tests.parade_case import CASES, load_parade_case


def _plugin(geom, P, S, **cfg):
    return PTParade(dict({"pretrained": geom}, **cfg), SimpleNamespace(config={"numpassages": P, "maxseqlen": S}))


def _model(name):
    c, enc, head, geom = load_parade_case(name)
    r = _plugin(geom, int(c["P"]), int(c["S"]))
    m = r.build_model()
    m.bert.load_state_dict(enc, strict=False)
    m.load_state_dict(head, strict=False)
    return c, r, m


@pytest.mark.parametrize("name", CASES)
def test_state_dict_names_and_shapes_match_the_reference(name):
    c, r, m = _model(name)
    sd = {k: v for k, v in m.state_dict().items() if not k.endswith("position_ids")}   # (a persistent buffer only in transformers 4.9)
    assert sorted(sd) == [str(k) for k in c["state_keys"]]
    for k, shape in zip(c["state_keys"], c["state_shapes"]):
        want = [int(x) for x in shape if x]
        assert list(sd[str(k)].shape) == want, k


def test_save_and_load_weights_round_trip(tmp_path):
    c, r, m = _model("parade_mini")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    fn = os.path.join(tmp_path, "w", "weights")
    r.save_weights(fn, opt)
    r2 = _plugin(load_parade_case("parade_mini")[3], int(c["P"]), int(c["S"]))
    m2 = r2.build_model()
    for p in m2.parameters():
        p.data.zero_()
    r2.load_weights(fn, torch.optim.Adam(m2.parameters(), lr=1e-3))
    a, b = m.state_dict(), m2.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_aggregations_the_reference_lacks_raise():
    geom = dict(hidden=64, layers=1, heads=1, ffn=128, vocab=200, max_pos=64)
    for agg in ("max", "avg", "attn"):
        with pytest.raises(NotImplementedError):
            _plugin(geom, 2, 32, aggregation=agg).build_model()
    with pytest.raises(ValueError):
        _plugin(geom, 2, 32, aggregation="mean").build_model()
    with pytest.raises(ValueError):
        _plugin("roberta-base", 2, 32).build_model()


def test_training_mode_raises():
    r = _plugin(dict(hidden=64, layers=1, heads=1, ffn=128, vocab=200, max_pos=64), 2, 32)
    m = r.build_model()
    m.train()
    x = torch.zeros((1, 2, 32), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="fine-tuning"):
        m(x, x, x)


def test_64_passages_are_refused_before_any_device_work():
    r = _plugin(dict(hidden=64, layers=1, heads=1, ffn=128, vocab=200, max_pos=64), 64, 32)
    m = r.build_model().eval()
    x = torch.zeros((1, 64, 32), dtype=torch.int64)      # (CPU tensors: any device work would raise RuntimeError instead)
    with pytest.raises(ValueError, match="passages"):
        m(x, x, x)
    assert m._engine is None
    from capreolus_amd import engine

    be = SimpleNamespace(skip_padding=True)
    with pytest.raises(ValueError, match="passages"):
        engine.ParadeEngine(be).forward(x, x, x, {})


def numpy_head(cls, B, P, head, eps=1e-12):
    """ptparade.py:53-65, 78 restated in float64: two post-LN BertLayers without a mask over [initial_cls; cls rows] + positions."""
    w = {k: v.detach().double().numpy() for k, v in head.items()}
    H = w["initial_cls_embedding"].size
    erf = np.vectorize(math.erf)

    def ln(x, g, b):
        mu = x.mean(-1, keepdims=True)
        var = ((x - mu) ** 2).mean(-1, keepdims=True)
        return (x - mu) / np.sqrt(var + eps) * g + b

    def layer(x, pre):
        p = lambda n: w[pre + n]
        lin = lambda t, n: t @ p(n + ".weight").T + p(n + ".bias")
        q, k, v = (lin(x, "attention.self." + n).reshape(B, P + 1, H // 64, 64).transpose(0, 2, 1, 3) for n in ("query", "key", "value"))
        s = q @ k.transpose(0, 1, 3, 2) / 8.0
        s = np.exp(s - s.max(-1, keepdims=True))
        ctx = ((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(B, P + 1, H)
        a = ln(lin(ctx, "attention.output.dense") + x, p("attention.output.LayerNorm.weight"), p("attention.output.LayerNorm.bias"))
        i = lin(a, "intermediate.dense")
        i = 0.5 * i * (1.0 + erf(i / math.sqrt(2.0)))
        return ln(lin(i, "output.dense") + a, p("output.LayerNorm.weight"), p("output.LayerNorm.bias"))

    x = np.concatenate([np.broadcast_to(w["initial_cls_embedding"].reshape(1, 1, H), (B, 1, H)), cls.astype(np.float64).reshape(B, P, H)], axis=1)
    x = x + w["full_position_embeddings"].reshape(1, P + 1, H)
    x = layer(layer(x, "transformer_layer_1."), "transformer_layer_2.")
    return x[:, 0] @ w["linear.weight"].reshape(H) + w["linear.bias"][0]


@pytest.mark.parametrize("name", CASES)
def test_numpy_head_on_the_reference_cls_rows_reproduces_the_reference_score(name):
    c, enc, head, geom = load_parade_case(name)
    B, P = c["pos_bert_input"].shape[:2]
    got = numpy_head(c["ref_cls"], B, P, head)
    ref = c["ref_score"].astype(np.float64)
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (got, ref)
