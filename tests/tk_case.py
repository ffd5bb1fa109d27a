"""TK fixtures (tests/golden/tk_*.npz, made by tests/golden/make_golden_tk.py from the reference TK_class): the numpy-seeded embedding
tables and weights both sides load, and the loader the tests use.  The .npz files hold only ids, configuration and reference outputs."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZERO_TOKEN = 7      # a non-pad token whose embedding row is all zeros (usemask treats it as padding; cosine does not)

# (a) defaults at the reproduction's shape; (b) usemask + usemixer, 1 layer of 6 heads of width 50; (c) a small model, 3 layers, Q = 8;
# (d) the gradient fixture of the training restatement (dropout p = 0 on both sides)
CASES = {
    "tk_default": dict(V=400, D=300, Q=4, L=800, B=6, seed=41, config={}),
    "tk_mask_mixer": dict(V=400, D=300, Q=4, L=200, B=6, seed=42, config={"usemask": True, "usemixer": True, "numlayers": 1, "numattheads": 6},
                          mixer=0.7),
    "tk_small": dict(V=300, D=50, Q=8, L=120, B=8, seed=43, config={"numattheads": 5, "numlayers": 3, "alpha": 0.2, "ffdim": 64}),
    "tk_grad": dict(V=300, D=50, Q=5, L=64, B=4, seed=44, config={"numattheads": 5, "usemask": True, "usemixer": True, "ffdim": 40}, mixer=0.6),
}
SCORE_CASES = ("tk_default", "tk_mask_mixer", "tk_small")
DEFAULTS = {"gradkernels": True, "scoretanh": False, "singlefc": True, "projdim": 32, "ffdim": 100, "numlayers": 2, "numattheads": 10,
            "alpha": 0.5, "usemask": False, "usemixer": False, "finetune": False}


def config(name):
    return dict(DEFAULTS, **CASES[name]["config"])


def embeddings(name):
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    emb = (rs.randn(c["V"], c["D"]) * 0.5).astype(np.float32)
    emb[0] = 0.0
    emb[ZERO_TOKEN] = 0.0
    return emb


def extractor(name):
    c = CASES[name]
    return SimpleNamespace(embeddings=embeddings(name), pad=0, config={"maxqlen": c["Q"], "maxdoclen": c["L"]})


def weights(name):
    """state_dict entries (numpy fp32) of a fixture's model, all but embedding.weight and position_encoder.pe.  Wider than the
    reference's init: the fcc weights at +-0.014 would bunch every score within ~1e-4; these spread them over many error bounds."""
    c, cfg = CASES[name], config(name)
    rs = np.random.RandomState(c["seed"] + 1000)
    D, Fd = c["D"], cfg["ffdim"]

    def n(*shape, s):
        return (rs.randn(*shape) * s).astype(np.float32)

    w = {}
    for i in range(cfg["numlayers"]):
        pre = f"transformer_encoder.layers.{i}."
        w[pre + "self_attn.in_proj_weight"] = n(3 * D, D, s=1.5 / D ** 0.5)
        w[pre + "self_attn.in_proj_bias"] = n(3 * D, s=0.1)
        w[pre + "self_attn.out_proj.weight"] = n(D, D, s=1.0 / D ** 0.5)
        w[pre + "self_attn.out_proj.bias"] = n(D, s=0.1)
        w[pre + "linear1.weight"] = n(Fd, D, s=1.0 / D ** 0.5)
        w[pre + "linear1.bias"] = n(Fd, s=0.1)
        w[pre + "linear2.weight"] = n(D, Fd, s=1.0 / Fd ** 0.5)
        w[pre + "linear2.bias"] = n(D, s=0.1)
        for k in ("norm1", "norm2"):
            w[pre + k + ".weight"] = 1.0 + n(D, s=0.1)
            w[pre + k + ".bias"] = n(D, s=0.1)
    w["mixer"] = np.full((1, 1, 1), c.get("mixer", 0.9), dtype=np.float32)
    w["s_log_fcc.weight"] = n(1, 11, s=0.5)
    w["s_len_fcc.weight"] = n(1, 11, s=0.5)
    w["comb_fcc.weight"] = np.array([[1.0, 0.7]], dtype=np.float32)
    return w


def inputs(name):
    """int64 query ids [B, Q] and document ids [B, L]: a document with trailing pads, a query with a pad, the zero-row token in a
    query and in documents, and (for all but the gradient case) an all-pad last document"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"] + 2000)
    B, Q, L, V = c["B"], c["Q"], c["L"], c["V"]
    q = rs.randint(1, V, size=(B, Q)).astype(np.int64)
    d = rs.randint(1, V, size=(B, L)).astype(np.int64)
    q[:, 0] = q[0, 0]                     # candidates of one query share terms
    d[:, : Q] = np.where(rs.rand(B, Q) < 0.5, q, d[:, :Q])
    d[0, L * 3 // 5:] = 0                 # trailing pads
    q[1, Q - 1] = 0                       # a query with a pad
    q[2, 1] = ZERO_TOKEN
    d[2, 3:L:7] = ZERO_TOKEN
    d[3, : L // 4] = ZERO_TOKEN
    if name != "tk_grad":
        d[B - 1] = 0                      # an all-pad document
    return q, d


def load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return {k: z[k] for k in z.files}


def build(name, plugin_cls):
    """(plugin, model) with the fixture's weights, on the CPU"""
    import torch

    r = plugin_cls(config(name), extractor(name))
    m = r.build_model()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights(name).items()}, strict=False)
    return r, m
