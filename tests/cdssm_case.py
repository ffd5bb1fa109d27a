"""CDSSM fixtures (tests/golden/cdssm_*.npz, made by tests/golden/make_golden_cdssm.py from the reference CDSSM_class): the
numpy-seeded embedding tables, weights and ids both sides load, and the loader the tests use.  The .npz files hold only ids,
configuration and reference outputs."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V, D = 64, 24

# each the smallest shape at which a distinct mistake shows: (default) the reference's defaults, 267 document windows; (multiple) both
# lengths are multiples of W, so both sides get a whole window of zeros, and the max runs over two filters, one bias positive and one
# negative; (one) a single token, a window that is mostly zeros; (cross) taps across a word boundary at dim 300; (negbias) every bias
# negative: the all-pad document's representation is all zero and its score exactly 0.5; (padrow) the table's row 0 is not zero: real
# pads are embedded, the appended ones are zeros; (grad) the gradient fixture of the training restatement
CASES = {
    "cdssm_default": dict(Q=4, L=800, B=6, seed=71, config={}),
    "cdssm_multiple": dict(Q=3, L=9, B=6, seed=72, config={"windowsize": 3, "nfilter": 2}, bias=(0.3, -0.2)),
    "cdssm_one": dict(Q=1, L=1, B=6, seed=73, config={}),
    "cdssm_cross": dict(Q=4, L=50, B=6, seed=74, D=300, config={"windowsize": 2, "nkernel": 5, "nfilter": 3}),
    "cdssm_negbias": dict(Q=4, L=20, B=6, seed=75, config={"nfilter": 2}, bias=(-0.05, -0.3)),
    "cdssm_padrow": dict(Q=4, L=20, B=6, seed=76, config={}, padrow=True),
    "cdssm_grad": dict(Q=4, L=20, B=6, seed=77, config={"nfilter": 2}),
}
SCORE_CASES = tuple(n for n in CASES if n != "cdssm_grad")
DEFAULTS = {"nkernel": 3, "nfilter": 1, "nhiddens": 30, "windowsize": 3, "dropoutrate": 0}


def config(name):
    return dict(DEFAULTS, **CASES[name]["config"])


def make_embeddings(rs, v=V, d=D, padrow=False):
    """[v, d] fp32 at scale 0.5; row 0 (the pad) all zeros unless padrow"""
    emb = (rs.randn(v, d) * 0.5).astype(np.float32)
    if not padrow:
        emb[0] = 0.0
    return emb


def embeddings(name):
    c = CASES[name]
    return make_embeddings(np.random.RandomState(c["seed"]), d=c.get("D", D), padrow=c.get("padrow", False))


def extractor(name):
    c = CASES[name]
    return SimpleNamespace(embeddings=embeddings(name), pad=0, config={"maxqlen": c["Q"], "maxdoclen": c["L"]})


def make_weights(rs, cfg, bias=None):
    """state_dict entries (numpy fp32) of a model, all but embedding.weight.  The taps are wide (scale 1) and the biases small, so that the
    maxima of different rows differ and the cosines of a case spread over many error bounds"""
    F, nk, nh = cfg["nfilter"], cfg["nkernel"], cfg["nhiddens"]
    w = {"conv.0.weight": rs.randn(F, 1, nk).astype(np.float32), "conv.0.bias": (rs.randn(F) * 0.1).astype(np.float32),
         "ffw.weight": (rs.randn(nh, nk) * 0.3).astype(np.float32), "ffw.bias": (rs.randn(nh) * 0.1).astype(np.float32)}
    if bias is not None:
        w["conv.0.bias"] = np.asarray(bias, dtype=np.float32)
    return w


def weights(name):
    """make_weights for a fixture (its own stream, seed + 1000)"""
    return make_weights(np.random.RandomState(CASES[name]["seed"] + 1000), config(name), CASES[name].get("bias"))


def make_ids(rs, B, Q, L, v=V):
    """int64 query ids [B, Q] and document ids [B, L] (B >= 5): every document draws from its own few terms, so that the maxima over
    its windows are its own; pair 1 has a padded tail (L >= 2), pair 3 a query of pads, the last pair a document of pads"""
    assert B >= 5, B
    q = rs.randint(1, v, size=(B, Q)).astype(np.int64)
    d = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        pool = rs.choice(np.arange(1, v), size=5, replace=False)
        d[b] = pool[rs.randint(0, len(pool), size=L)]
    d[1, (L + 1) // 2:] = 0
    q[3] = 0
    d[B - 1] = 0
    return q, d


def check_ids(q, d):
    """the edge patterns the tests rely on"""
    B, L = d.shape
    assert (d[B - 1] == 0).all() and (q[B - 1] != 0).all() and (q[3] == 0).all() and (d[3] != 0).all()
    assert (d[1, (L + 1) // 2:] == 0).all() and (d[1, :(L + 1) // 2] != 0).all()


def inputs(name):
    """make_ids for a fixture (its own stream, seed + 2000); the gradient case draws a second set of documents as the negatives"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"] + 2000)
    q, d = make_ids(rs, c["B"], c["Q"], c["L"])
    if name == "cdssm_grad":
        return q, d, rs.randint(0, V, size=d.shape).astype(np.int64)
    return q, d


# every (Q, L, windowsize, nkernel, nfilter, dim) of the sweep of the device tests: lengths on both sides of a multiple of the window
# (and exactly on it), windows of 1 .. 4 terms, nkernel 1, 3 and windowsize x dim (one output, R = 1), one filter and several, more
# windows than the four waves of a workgroup, more outputs than a wave's 64 lanes, and both instantiations of the tower kernel (dim a
# multiple of 4: rows read as float4; any other dim: as floats); the last point is every limit at once (dim 512, windowsize 8, nkernel 16,
# nfilter 16): 128 KiB of LDS, the one geometry class that has to ask for more than a kernel gets by default
SWEEP = (
    (4, 11, 1, 1, 1, 24), (3, 12, 1, 3, 2, 23),
    (4, 12, 2, 3, 2, 24), (5, 13, 2, 3, 1, 23), (3, 11, 2, 1, 3, 24),
    (3, 9, 3, 3, 1, 24), (4, 10, 3, 3, 3, 23), (5, 50, 3, 3, 2, 24), (2, 8, 3, 1, 1, 23),
    (4, 17, 4, 3, 2, 24), (7, 16, 4, 1, 1, 23), (8, 15, 4, 3, 1, 24),
    (3, 7, 3, 15, 2, 5), (4, 9, 4, 16, 1, 4), (2, 5, 2, 10, 3, 5),
    (2, 17, 8, 16, 16, 512),
)


def sweep_case(Q, L, W, nk, F, dim):
    """(config, extractor, weights, query ids [3, Q], document ids [3, L]) of a sweep point, all from one stream seeded by the point:
    a table whose row 0 is NOT zero; a random document, one with a padded tail, one of pads"""
    rs = np.random.RandomState(((((Q * 101 + L) * 11 + W) * 17 + nk) * 5 + F) * 7 + dim % 7)
    cfg = dict(DEFAULTS, windowsize=W, nkernel=nk, nfilter=F)
    ex = SimpleNamespace(embeddings=make_embeddings(rs, V, dim, padrow=True), pad=0, config={"maxqlen": Q, "maxdoclen": L})
    w = make_weights(rs, cfg)
    q = rs.randint(1, V, size=(3, Q)).astype(np.int64)
    d = rs.randint(1, V, size=(3, L)).astype(np.int64)
    q[1, Q - 1] = 0
    d[1, L // 2:] = 0
    d[2] = 0
    return cfg, ex, w, q, d


def sweep_key(Q, L, W, nk, F, dim):
    return f"{Q}.{L}.{W}.{nk}.{F}.{dim}"


def load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return {k: z[k] for k in z.files}


def build(name, plugin_cls):
    """(plugin, model) with the fixture's weights, on the CPU"""
    return build_from(config(name), extractor(name), weights(name), plugin_cls)


def build_from(cfg, ex, w, plugin_cls):
    import torch

    r = plugin_cls(cfg, ex)
    m = r.build_model()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    return r, m
