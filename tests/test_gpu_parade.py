"""PARADE (reranker `ptparade`) on the GPU: the fp32 aggregation head (csrc/parade.hip) on the reference's own [CLS] rows, the whole
model against the reference's fixtures (tests/golden/parade_*.npz) in fp16 and bf16, its invariances, and the predict path."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from capreolus_amd import engine
from capreolus_amd.reranker import PTParade
from tests.parade_case import CASES, load_parade_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the end-to-end bound: this factor times the reference's own autocast error (ref_score_amp_* against ref_score) + 1e-4, as
# test_bert_maxp_end_to_end does, and never more than the fixed cap (what the fixtures' autocast errors allow, with room)
E2E = {"fp16": (1.25, 0.08), "bf16": (1.5, 1.0)}


def _head_dev(head):
    return {k: v.to(DEV) for k, v in head.items()}


def torch_head(cls, B, P, head, eps=1e-12):
    """ptparade.py:53-65, 78 in plain PyTorch (float64 on the device): two post-LN BertLayers, no mask, then `linear` on row 0."""
    w = {k: v.double() for k, v in head.items()}
    H = w["initial_cls_embedding"].numel()
    x = torch.cat([w["initial_cls_embedding"].view(1, 1, H).expand(B, 1, H), cls.double().view(B, P, H)], 1) + w["full_position_embeddings"]
    ln = lambda t, pre: torch.nn.functional.layer_norm(t, (H,), w[pre + ".weight"], w[pre + ".bias"], eps)
    for layer in ("transformer_layer_1.", "transformer_layer_2."):
        lin = lambda t, n: t @ w[layer + n + ".weight"].T + w[layer + n + ".bias"]
        q, k, v = (lin(x, "attention.self." + n).view(B, P + 1, H // 64, 64).transpose(1, 2) for n in ("query", "key", "value"))
        ctx = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v
        a = ln(lin(ctx.transpose(1, 2).reshape(B, P + 1, H), "attention.output.dense") + x, layer + "attention.output.LayerNorm")
        x = ln(lin(torch.nn.functional.gelu(lin(a, "intermediate.dense")), "output.dense") + a, layer + "output.LayerNorm")
    return x[:, 0] @ w["linear.weight"].view(H) + w["linear.bias"][0]


@pytest.mark.parametrize("name", CASES)
def test_head_on_the_reference_cls_rows(name):
    c, enc, head, geom = load_parade_case(name)
    B, P = c["pos_bert_input"].shape[:2]
    pe = engine.ParadeEngine(None)
    got = pe.head(torch.from_numpy(c["ref_cls"]).to(DEV), B, P, _head_dev(head)).cpu().numpy().astype(np.float64)
    ref = c["ref_score"].astype(np.float64)
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (got, ref)


@pytest.mark.parametrize("B", [16, 1])
def test_head_at_benchmark_scale(B):
    from tests.parade_case import parade_head_weights

    P, H, F = 16, 768, 3072
    head = _head_dev(parade_head_weights(5, H, F, P))
    cls = torch.randn(B * P, H, generator=torch.Generator().manual_seed(B)).to(DEV)
    pe = engine.ParadeEngine(None)
    got, agg = pe.head(cls, B, P, head, aggregated=True)
    want = torch_head(cls, B, P, head)
    assert (got.double() - want).abs().max().item() <= 1e-5 * max(1.0, want.abs().max().item())
    assert torch.allclose(agg.double() @ head["linear.weight"].double().view(H) + head["linear.bias"].double(), got.double(), atol=1e-4)


def test_head_refuses_geometries_it_does_not_compute():
    from tests.parade_case import parade_head_weights

    pe = engine.ParadeEngine(None)
    cls = torch.zeros(4 * 64, 128, device=DEV)
    with pytest.raises(ValueError):
        pe.head(cls, 4, 64, _head_dev(parade_head_weights(1, 128, 256, 64)))        # P + 1 = 65 rows
    with pytest.raises(ValueError):
        pe.head(cls[:8], 4, 2, _head_dev(parade_head_weights(1, 128, 256, 3)))       # position table of another P


def _plugin(name, dt, **cfg):
    c, enc, head, geom = load_parade_case(name)
    P, S = int(c["P"]), int(c["S"])
    r = PTParade(dict({"pretrained": geom, "compute_dtype": dt}, **cfg), SimpleNamespace(config={"numpassages": P, "maxseqlen": S}))
    m = r.build_model()
    m.bert.load_state_dict(enc, strict=False)
    m.load_state_dict(head, strict=False)
    m.to(DEV).eval()
    d = {"pos_bert_input": torch.from_numpy(c["pos_bert_input"].astype(np.int64)).to(DEV),
         "pos_mask": torch.from_numpy(c["pos_mask"].astype(np.int64)).to(DEV), "pos_seg": torch.from_numpy(c["pos_seg"].astype(np.int64)).to(DEV)}
    return c, r, d


@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_parade_end_to_end(name, dt):
    c, r, d = _plugin(name, dt)
    with torch.no_grad():
        got = r.test(d).cpu().numpy().astype(np.float64)
    ref = c["ref_score"].astype(np.float64)
    factor, cap = E2E[dt]
    bound = factor * np.abs(c[f"ref_score_amp_{dt}"] - ref).max() + 1e-4
    err = np.abs(got - ref).max()
    assert err <= bound and err <= cap, (name, dt, err, bound, got, ref)
    for i in range(len(ref)):           # reference order kept wherever it is decided by more than twice the bound
        for j in range(len(ref)):
            if ref[i] - ref[j] > 2 * bound:
                assert got[i] > got[j], (i, j, got, ref)


def test_parade_cls_rows_match_the_reference():
    c, r, d = _plugin("parade_base", "fp16")
    with torch.no_grad():
        _, cls = r.model.engine().forward(d["pos_bert_input"], d["pos_mask"], d["pos_seg"], r.model.head_params(), return_cls=True)
    ref = c["ref_cls"]
    assert np.abs(cls.cpu().numpy() - ref).max() <= 2e-2 * np.abs(ref).max()


@pytest.mark.parametrize("name", ["parade_mini", "parade_base"])
def test_skip_padding_and_batch_composition_do_not_change_a_score(name):
    c, r, d = _plugin(name, "fp16")
    m = r.model
    ids, mask, seg = d["pos_bert_input"], d["pos_mask"], d["pos_seg"]
    eng = m.engine()
    with torch.no_grad():
        on = eng.forward(ids, mask, seg, m.head_params(), skip_padding=True)
        off = eng.forward(ids, mask, seg, m.head_params(), skip_padding=False)
        assert torch.equal(on, off)
        B = ids.shape[0]
        h = B // 2
        two = torch.cat([eng.forward(ids[:h], mask[:h], seg[:h], m.head_params()), eng.forward(ids[h:], mask[h:], seg[h:], m.head_params())])
        assert torch.equal(two, on)
        rev = eng.forward(ids.flip(0), mask.flip(0), seg.flip(0), m.head_params()).flip(0)
        assert torch.equal(rev, on)


def test_predict_equals_test():
    from capreolus_amd.trainer.pytorch import PytorchTrainer

    c, r, d = _plugin("parade_mini", "fp16")
    host = {k: v.cpu().numpy() for k, v in d.items()}
    B = host["pos_bert_input"].shape[0]
    q2d = {"q1": [f"d{i}" for i in range(3)], "q2": [f"d{i}" for i in range(3, B)]}

    class Sampler(torch.utils.data.IterableDataset):
        qid_to_docids = q2d

        def __iter__(self):
            for qid, docs in self.qid_to_docids.items():
                for doc in docs:
                    i = int(doc[1:])
                    yield {"qid": qid, "posdocid": doc, **{k: v[i] for k, v in host.items()}}

        def __len__(self):
            return B

        def get_qid_docid_pairs(self):
            return ((q, doc) for q, docs in self.qid_to_docids.items() for doc in docs)

    preds = PytorchTrainer({"batch": 2}).predict(r, Sampler())
    with torch.no_grad():
        direct = r.test(d).cpu().numpy().astype(np.float16)
    for q, docs in q2d.items():
        for doc in docs:
            assert preds[q][doc] == float(direct[int(doc[1:])]), (q, doc)
