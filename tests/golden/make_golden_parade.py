"""PARADE golden vectors: the REFERENCE PTParade_Class (capreolus/reranker/ptparade.py, imported from the reference tree through
_refharness) driving transformers' BertModel / ElectraModel and two BertLayers, on seeded encoder weights
(oracle.bert_port.random_weights), seeded head weights (tests/parade_case.py) and seeded BertPassage-shaped inputs.  Build container
only; data out, no code.

    python tests/golden/make_golden_parade.py            (from the repository root)
"""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from capreolus_amd import synthetic  # noqa: E402
from oracle import bert_port  # noqa: E402
from tests.parade_case import parade_head_weights  # noqa: E402

CASES = {
    "parade_mini": dict(arch="bert", hidden=128, layers=2, heads=2, ffn=512, vocab=1000, max_pos=128, B=5, P=3, S=64, seed=21),
    "parade_electra_mini": dict(arch="electra", hidden=128, layers=2, heads=2, ffn=256, vocab=1000, max_pos=128, B=4, P=5, S=64, seed=22),
    # the reproduction's shape per document (16 passages x 256 tokens), empty passages, and a document that is mostly padding passages
    "parade_base": dict(arch="bert", hidden=768, layers=12, heads=12, ffn=3072, vocab=30522, max_pos=512, B=3, P=16, S=256, seed=23,
                        pad_doc=True),
}
FP16_REL = 1.25   # the end-to-end bound of tests/test_gpu_parade.py: 1.25 x the reference's own fp16 autocast error + 1e-4
# the scores of a fixture spread over at least this many end-to-end fp16 bounds (the reference's own fp16 error is ~2 % of the spread
# on these encoders, whatever the head weights: 50 bounds, as first planned, is out of reach; 25 leaves the rank checks many pairs)
SPREAD = 25


def _one_tuple(layer):
    """transformers 5.x BertLayer returns a tensor; the reference unpacks a 1-tuple (ptparade.py:62-63).  Same arithmetic."""
    fwd = layer.forward

    def wrapped(*a, **k):
        out = fwd(*a, **k)
        return (out,) if torch.is_tensor(out) else out

    layer.forward = wrapped


def gen(name, c, PARADE):
    from transformers import BertConfig, BertModel, ElectraConfig, ElectraModel

    H, P, S, B = c["hidden"], c["P"], c["S"], c["B"]
    kw = dict(hidden_size=H, num_hidden_layers=c["layers"], num_attention_heads=c["heads"], intermediate_size=c["ffn"], vocab_size=c["vocab"],
              max_position_embeddings=c["max_pos"])
    electra = c["arch"] == "electra"
    cfg = ElectraConfig(embedding_size=H, **kw) if electra else BertConfig(**kw)
    Model = ElectraModel if electra else BertModel
    w = bert_port.random_weights(H, c["layers"], c["heads"], c["ffn"], c["vocab"], c["max_pos"], seed=c["seed"])
    orig = Model.from_pretrained
    Model.from_pretrained = staticmethod(lambda *a, **k: Model(cfg))
    try:
        rs = np.random.RandomState(c["seed"])
        batch = synthetic.make_bert_passages(rs, B, P, S, vocab=c["vocab"], same_query=False)
        if c.get("pad_doc"):       # the last document: 3 real passages, the rest the extractor's padding passages ([CLS] q [SEP] [PAD] [SEP])
            for k in ("pos_bert_input", "pos_mask", "pos_seg"):
                t = batch[k]
                nq = int((batch["pos_seg"][B - 1, 0] == 0).sum()) - 2
                pad = np.zeros(S, dtype=t.dtype)
                if k == "pos_bert_input":
                    pad[:nq + 4] = [101] + list(batch[k][B - 1, 0, 1:nq + 1]) + [102, 0, 102]
                elif k == "pos_mask":
                    pad[:nq + 4] = 1
                    pad[nq + 2] = 0
                else:
                    pad[nq + 2:] = 1
                t[B - 1, 3:] = pad
        ti = {k: torch.from_numpy(v) for k, v in batch.items()}
        model = PARADE.PTParade_Class(SimpleNamespace(config={"numpassages": P, "maxseqlen": S}),
                                      {"pretrained": "electra-base-msmarco" if electra else "bert-base-uncased", "aggregation": "transformer"})
        enc = {k[5:]: v for k, v in w.items() if k.startswith("bert.") and not (electra and k.startswith("bert.pooler."))}
        missing = model.bert.load_state_dict(enc, strict=False)
        assert not [k for k in missing.missing_keys if "position_ids" not in k], missing
        assert not missing.unexpected_keys, missing
        head = parade_head_weights(c["seed"], H, c["ffn"], P, w["bert.embeddings.word_embeddings.weight"])
        sd = model.state_dict()
        for k, v in head.items():
            assert sd[k].shape == v.shape, (k, sd[k].shape, v.shape)
        missing = model.load_state_dict(head, strict=False)
        assert not missing.unexpected_keys and not [k for k in missing.missing_keys if not k.startswith("bert.")], missing
        _one_tuple(model.transformer_layer_1)
        _one_tuple(model.transformer_layer_2)
        model.eval()
        ids, mask, seg = ti["pos_bert_input"], ti["pos_mask"], ti["pos_seg"]
        with torch.no_grad():
            # centre the scores: the documents share a large common component of linear(X2[b][0]), and under autocast the score
            # itself is rounded to 16 bits - at |score| ~ 9 that rounding alone would be most of the reference's fp16 error
            bias = float(np.round(float(model.linear.bias) - model(ids, mask, seg).view(-1).mean().item(), 3))
            model.linear.bias.fill_(bias)
            ref = model(ids, mask, seg).view(-1).numpy().astype(np.float32)
            cls = model.bert(ids.view(B * P, S), attention_mask=mask.view(B * P, S), token_type_ids=seg.view(B * P, S))[0][:, 0, :]
            again = model.linear(model.aggregation(cls)).view(-1).numpy()
            assert np.array_equal(again, ref), (again, ref)
            amp = {}
            for dt, tag in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
                with torch.autocast("cpu", dtype=dt):         # the reference's amp = pred mode, on the CPU
                    amp[tag] = model(ids, mask, seg).view(-1).float().numpy()
    finally:
        Model.from_pretrained = orig
    err16 = float(np.abs(amp["fp16"] - ref).max())
    spread = float(ref.max() - ref.min())
    tol16 = FP16_REL * err16 + 1e-4
    assert spread >= SPREAD * tol16, (name, spread, tol16)
    keys = sorted(k for k in model.state_dict() if not k.endswith("position_ids"))
    shapes = np.array([list(model.state_dict()[k].shape) + [0] * (3 - model.state_dict()[k].dim()) for k in keys], dtype=np.int64)
    np.savez_compressed(
        os.path.join(HERE, f"{name}.npz"), weight_seed=np.int64(c["seed"]),
        dims=np.array([H, c["layers"], c["heads"], c["ffn"], c["vocab"], c["max_pos"]], dtype=np.int64), P=np.int64(P), S=np.int64(S),
        pooler=np.bool_(not electra), arch=np.array(c["arch"]),
        pos_bert_input=batch["pos_bert_input"].astype(np.int32), pos_mask=batch["pos_mask"].astype(np.int8), pos_seg=batch["pos_seg"].astype(np.int8),
        ref_score=ref, ref_cls=cls.numpy().astype(np.float32), ref_score_amp_fp16=amp["fp16"].astype(np.float32),
        ref_score_amp_bf16=amp["bf16"].astype(np.float32), linear_bias=np.float32(bias), state_keys=np.array(keys), state_shapes=shapes)
    print(name, "scores", ref, "fp16 err", err16, "bf16 err", float(np.abs(amp["bf16"] - ref).max()), "spread", spread)


def main(only=None):
    import _refharness

    _refharness.load_reference()
    PARADE = importlib.import_module("capreolus.reranker.ptparade")
    for name, c in CASES.items():
        if not only or name in only:
            gen(name, c, PARADE)


if __name__ == "__main__":
    main(sys.argv[1:])
