"""PARADE fixtures (tests/golden/parade_*.npz, made by tests/golden/make_golden_parade.py): the seeded aggregation-head weights the
generator loads into the reference PTParade_Class, and the loader the tests use.  Encoder weights are oracle.bert_port.random_weights."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("parade_mini", "parade_electra_mini", "parade_base")
LAYER_TENSORS = (
    "attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight", "attention.self.key.bias",
    "attention.self.value.weight", "attention.self.value.bias", "attention.output.dense.weight", "attention.output.dense.bias",
    "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias",
    "output.dense.weight", "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias",
)


def parade_head_weights(seed, hidden, ffn, P, word_emb=None):
    """Seeded head of a PARADE fixture under PTParade_Class's state_dict names (torch fp32 CPU tensors).  Wider than the reference's
    init (BertLayer 0.02, position embeddings 0.02), with non-trivial LayerNorm / bias terms and a wide `linear`, so that the
    attention mixes the passages and the documents' scores spread (with the reference's init BERT-base scores differ only in the
    third decimal, and a rank check would be vacuous).  initial_cls_embedding = word embedding row 101, as the reference sets it."""
    import torch

    g = torch.Generator().manual_seed(seed + 2000)

    def n(*shape, s=0.05):
        return torch.randn(*shape, generator=g) * s

    H, F = hidden, ffn
    w = {"initial_cls_embedding": (word_emb[101].clone() if word_emb is not None else n(H)).view(1, H),
         "full_position_embeddings": n(1, P + 1, H, s=0.1)}
    shapes = {"attention.self.query": (H, H), "attention.self.key": (H, H), "attention.self.value": (H, H), "attention.output.dense": (H, H),
              "intermediate.dense": (F, H), "output.dense": (H, F)}
    for layer in (1, 2):
        pre = f"transformer_layer_{layer}."
        for name in LAYER_TENSORS:
            mod, kind = name.rsplit(".", 1)
            if "LayerNorm" in mod:
                w[pre + name] = (1.0 + n(H, s=0.1)) if kind == "weight" else n(H, s=0.1)
            else:
                rows, cols = shapes[mod]
                w[pre + name] = n(rows, cols, s=1.0 / cols ** 0.5) if kind == "weight" else n(rows, s=0.1)
    w["linear.weight"] = n(1, H, s=1.0)
    w["linear.bias"] = n(1, s=0.1)
    return w


def load_parade_case(name):
    """(fixture dict, encoder weights, head weights, encoder geometry for bert_body) of a PARADE fixture."""
    import torch

    from oracle import bert_port

    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    c = {k: z[k] for k in z.files}
    hidden, layers, heads, ffn, vocab, max_pos = (int(x) for x in c["dims"])
    P = int(c["P"])
    w = bert_port.random_weights(hidden, layers, heads, ffn, vocab, max_pos, seed=int(c["weight_seed"]))
    pooler = bool(c["pooler"])
    enc = {k[len("bert."):]: v for k, v in w.items() if k.startswith("bert.") and (pooler or not k.startswith("bert.pooler."))}
    head = parade_head_weights(int(c["weight_seed"]), hidden, ffn, P, w["bert.embeddings.word_embeddings.weight"])
    head["linear.bias"] = torch.tensor([float(c["linear_bias"])])   # the generator centres the scores (make_golden_parade.py)
    geom = dict(hidden=hidden, layers=layers, heads=heads, ffn=ffn, vocab=vocab, max_pos=max_pos, pooler=pooler)
    return c, enc, head, geom
