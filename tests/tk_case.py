"""TK fixtures (tests/golden/tk_*.npz, made by tests/golden/make_golden_tk.py from the reference TK_class): the numpy-seeded embedding
tables and weights both sides load, and the loader the tests use.  The .npz files hold only ids, configuration and reference outputs."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZERO_TOKEN = 7      # a non-pad token whose embedding row is all zeros (usemask treats it as padding; cosine does not)

# (a) defaults at the reproduction's shape; (b) usemask + usemixer, 1 layer of 6 heads of width 50; (c) a small model, 3 layers, Q = 8;
# (d) the gradient fixture of the training restatement (dropout p = 0 on both sides); (e) head width 40 (slot 48), ffdim 192 (the ReLU
# GEMM's 3-block tiles), Q = 12 (two pooling chunks of query rows), pads mid-document; (f) usemask + usemixer at L = 300 with the
# dead-tile documents of `ids` (two whole 64-key tiles masked before the first live key, one live key, none) and a query of zero rows
CASES = {
    "tk_default": dict(V=400, D=300, Q=4, L=800, B=6, seed=41, config={}),
    "tk_mask_mixer": dict(V=400, D=300, Q=4, L=200, B=6, seed=42, config={"usemask": True, "usemixer": True, "numlayers": 1, "numattheads": 6},
                          mixer=0.7),
    "tk_small": dict(V=300, D=50, Q=8, L=120, B=8, seed=43, config={"numattheads": 5, "numlayers": 3, "alpha": 0.2, "ffdim": 64}),
    "tk_grad": dict(V=300, D=50, Q=5, L=64, B=4, seed=44, config={"numattheads": 5, "usemask": True, "usemixer": True, "ffdim": 40}, mixer=0.6),
    "tk_heads48": dict(V=400, D=200, Q=12, L=130, B=6, seed=45, config={"numattheads": 5, "ffdim": 192}, mid_pads=True),
    "tk_mask_tiles": dict(V=400, D=128, Q=9, L=300, B=8, seed=46, config={"usemask": True, "usemixer": True, "numattheads": 4, "ffdim": 256},
                          mixer=0.6, mid_pads=True, dead_tiles=True),
}
SCORE_CASES = ("tk_default", "tk_mask_mixer", "tk_small", "tk_heads48", "tk_mask_tiles")
DEFAULTS = {"gradkernels": True, "scoretanh": False, "singlefc": True, "projdim": 32, "ffdim": 100, "numlayers": 2, "numattheads": 10,
            "alpha": 0.5, "usemask": False, "usemixer": False, "finetune": False}


def config(name):
    return dict(DEFAULTS, **CASES[name]["config"])


def make_embeddings(rs, V, D):
    """[V, D] fp32 at scale 0.5; row 0 (the pad) and row ZERO_TOKEN all zeros"""
    emb = (rs.randn(V, D) * 0.5).astype(np.float32)
    emb[0] = 0.0
    emb[ZERO_TOKEN] = 0.0
    return emb


def embeddings(name):
    c = CASES[name]
    return make_embeddings(np.random.RandomState(c["seed"]), c["V"], c["D"])


def extractor(name):
    c = CASES[name]
    return SimpleNamespace(embeddings=embeddings(name), pad=0, config={"maxqlen": c["Q"], "maxdoclen": c["L"]})


def make_weights(rs, D, Fd, numlayers, mixer=0.9):
    """state_dict entries (numpy fp32) of a model, all but embedding.weight and position_encoder.pe.  Wider than the reference's init:
    the fcc weights at +-0.014 would bunch every score within ~1e-4; these spread them over many error bounds."""

    def n(*shape, s):
        return (rs.randn(*shape) * s).astype(np.float32)

    w = {}
    for i in range(numlayers):
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
    w["mixer"] = np.full((1, 1, 1), mixer, dtype=np.float32)
    w["s_log_fcc.weight"] = n(1, 11, s=0.5)
    w["s_len_fcc.weight"] = n(1, 11, s=0.5)
    w["comb_fcc.weight"] = np.array([[1.0, 0.7]], dtype=np.float32)
    return w


def weights(name):
    """make_weights for a fixture (its own stream, seed + 1000)"""
    c, cfg = CASES[name], config(name)
    return make_weights(np.random.RandomState(c["seed"] + 1000), c["D"], cfg["ffdim"], cfg["numlayers"], c.get("mixer", 0.9))


def make_ids(rs, B, Q, L, V, all_pad_doc=True, mid_pads=False, dead_tiles=False):
    """int64 query ids [B, Q] and document ids [B, L]: random ids, candidates sharing query terms, a document with trailing pads, a
    query with a pad, the zero-row token in a query and in documents, and (all_pad_doc) an all-pad last document.  The options add,
    after every draw the base layout makes (so they leave its stream alone):
      mid_pads:   pads inside document 1 (a run and every 11th position) and zero-row tokens inside document 0's live part;
      dead_tiles: (B >= 8) document 4 of zero-row tokens over its first min(130, L - 1) positions (usemask: two whole 64-key tiles dead
                  before the first live key), document 5 of zero-row tokens only, document 6 of zero-row tokens but one position
                  (past 128 where L allows: a single live key in the third tile), and query 6 of zero-row tokens and pads only."""
    q = rs.randint(1, V, size=(B, Q)).astype(np.int64)
    d = rs.randint(1, V, size=(B, L)).astype(np.int64)
    q[:, 0] = q[0, 0]                     # candidates of one query share terms
    n = min(Q, L)
    d[:, :n] = np.where(rs.rand(B, n) < 0.5, q[:, :n], d[:, :n])
    d[0, L * 3 // 5:] = 0                 # trailing pads
    if B > 1:
        q[1, Q - 1] = 0                   # a query with a pad
    if B > 2:
        q[2, min(1, Q - 1)] = ZERO_TOKEN
        d[2, 3:L:7] = ZERO_TOKEN
    if B > 3:
        d[3, : L // 4] = ZERO_TOKEN
    if mid_pads and B > 1:
        d[1, L // 3: L // 3 + max(1, L // 10)] = 0
        d[1, 1:L:11] = 0
        d[0, 2: L * 3 // 5: 13] = ZERO_TOKEN
    if dead_tiles:
        assert B >= 8, B
        d[4, : min(130, L - 1)] = ZERO_TOKEN
        d[5] = ZERO_TOKEN
        d[6] = ZERO_TOKEN
        d[6, min(L - 1, 150)] = rs.randint(ZERO_TOKEN + 1, V)
        q[6] = np.where(np.arange(Q) % 2 == 0, ZERO_TOKEN, 0)
    if all_pad_doc:
        d[B - 1] = 0                      # an all-pad document
    return q, d


def inputs(name):
    """make_ids for a fixture (its own stream, seed + 2000); every case but the gradient one has an all-pad last document"""
    c = CASES[name]
    return make_ids(np.random.RandomState(c["seed"] + 2000), c["B"], c["Q"], c["L"], c["V"], all_pad_doc=name != "tk_grad",
                    mid_pads=c.get("mid_pads", False), dead_tiles=c.get("dead_tiles", False))


def load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return {k: z[k] for k in z.files}


def build(name, plugin_cls):
    """(plugin, model) with the fixture's weights, on the CPU"""
    return build_from(config(name), extractor(name), weights(name), plugin_cls)


def build_from(cfg, ex, w, plugin_cls):
    """(plugin, model) of a full config, an extractor and make_weights' entries, on the CPU"""
    import torch

    r = plugin_cls(cfg, ex)
    m = r.build_model()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    return r, m
