"""HINT fixtures (tests/golden/hint_*.npz, made by tests/golden/make_golden_hint.py from the reference HiNT_main): the numpy-seeded
embedding tables, weights and ids both sides load, and the loader the tests use.  The .npz files hold only ids, configuration and
reference outputs."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V, D = 64, 24
TINY_TOKEN = 5      # a token whose embedding row has norm ~1e-7: the wrong epsilon or a product-of-norms denominator changes its cosines

# each the smallest shape at which a distinct mistake shows: (small) P = 2 with an odd Q: row order and reversal; (default) the reference's
# defaults; (tail) kmax = 2P exactly and 50 tail terms that must be ignored; (one) a single row, a single window, LSTM length 1;
# (grad) the gradient fixture of the training restatement
CASES = {
    "hint_small": dict(Q=3, L=200, B=6, seed=61, config={"kmax": 3}),
    "hint_default": dict(Q=4, L=800, B=5, seed=62, config={}),
    "hint_tail": dict(Q=5, L=250, B=5, seed=63, config={"kmax": 4}),
    "hint_one": dict(Q=1, L=100, B=5, seed=64, config={"kmax": 1}),
    "hint_grad": dict(Q=3, L=200, B=5, seed=65, config={"kmax": 3}),
    # both limits of the front end at once: 32 query rows of 512 floats are 64 KiB + 256 bytes of LDS, the one geometry that has to
    # ask for more than a kernel gets by default
    "hint_wide": dict(Q=32, L=200, B=5, seed=66, D=512, config={"kmax": 2}),
}
SCORE_CASES = ("hint_small", "hint_default", "hint_tail", "hint_one", "hint_wide")
DEFAULTS = {"spatialGRU": 2, "LSTMdim": 6, "kmax": 10}


def config(name):
    return dict(DEFAULTS, **CASES[name]["config"])


def make_embeddings(rs, v=V, d=D):
    """[v, d] fp32 at scale 0.5; row 0 (the pad) all zeros, row TINY_TOKEN of norm ~1e-7"""
    emb = (rs.randn(v, d) * 0.5).astype(np.float32)
    emb[0] = 0.0
    emb[TINY_TOKEN] = (emb[TINY_TOKEN] / np.linalg.norm(emb[TINY_TOKEN]) * 1e-7).astype(np.float32)
    return emb


def embeddings(name):
    return make_embeddings(np.random.RandomState(CASES[name]["seed"]), d=CASES[name].get("D", D))


def extractor(name):
    c = CASES[name]
    return SimpleNamespace(embeddings=embeddings(name), pad=0, config={"maxqlen": c["Q"], "maxdoclen": c["L"]})


def make_weights(rs, d, kmax):
    """state_dict entries (numpy fp32) of a model, all but HiNT1.embedding.weight; wide enough that the gates leave their linear range
    and the scores of a case spread over many error bounds"""

    def n(*shape, s):
        return (rs.randn(*shape) * s).astype(np.float32)

    w = {"HiNT1.Ws.weight": n(1, d, s=1.0 / d ** 0.5), "HiNT1.Ws.bias": n(1, s=0.2)}
    for g in ("GRU2d1", "GRU2d3"):
        pre = f"HiNT1.{g}.gru_cell."
        w[pre + "Wrz.weight"], w[pre + "Wrz.bias"] = n(14, 9, s=0.7), n(14, s=0.3)
        w[pre + "W.weight"], w[pre + "W.bias"] = n(2, 3, s=0.7), n(2, s=0.3)
        w[pre + "U.weight"], w[pre + "U.bias"] = n(2, 6, s=0.7), n(2, s=0.3)
    for rev in ("", "_reverse"):
        w[f"HiNT1.lstm.weight_ih_l0{rev}"], w[f"HiNT1.lstm.weight_hh_l0{rev}"] = n(24, 8, s=0.6), n(24, 6, s=0.6)
        w[f"HiNT1.lstm.bias_ih_l0{rev}"], w[f"HiNT1.lstm.bias_hh_l0{rev}"] = n(24, s=0.2), n(24, s=0.2)
    w["HiNT1.Wv.weight"], w["HiNT1.Wv.bias"] = n(6, 8, s=0.6), n(6, s=0.2)
    w["HiNT1.fc.weight"], w["HiNT1.fc.bias"] = n(1, 6 * kmax, s=0.5), n(1, s=0.2)
    return w


def weights(name):
    """make_weights for a fixture (its own stream, seed + 1000)"""
    return make_weights(np.random.RandomState(CASES[name]["seed"] + 1000), CASES[name].get("D", D), config(name)["kmax"])


def make_ids(rs, B, Q, L, v=V):
    """int64 query ids [B, Q] and document ids [B, L] (B >= 5) with the patterns check_ids asserts"""
    assert B >= 5, B
    P = L // 100
    q = rs.randint(1, v, size=(B, Q)).astype(np.int64)
    d = rs.randint(1, v, size=(B, L)).astype(np.int64)
    q[q == TINY_TOKEN] = TINY_TOKEN + 1
    # pair 0: exact matches in column 0 and column 99 of the first window and in column 99 of the last
    d[0, 0], d[0, 99], d[0, P * 100 - 1] = q[0, 0], q[0, Q - 1], q[0, 0]
    # pair 1: a padded query term against real terms (not masked) and against a padded document tail (the both-pad mask)
    q[1, Q - 1] = 0
    d[1, L // 2:] = 0
    # pair 2: a repeated query term, the tiny-norm row in the query (Q > 1) and in the document
    q[2, Q - 1] = q[2, 0]
    if Q > 1:
        q[2, 1 if Q > 2 else 0] = TINY_TOKEN
        q[2, Q - 1] = q[2, 0]
    d[2, 3:L:7] = TINY_TOKEN
    d[2, 1] = q[2, 0]
    # pair 3: a query of all pads against a document with pads inside
    q[3] = 0
    d[3, 10:20] = 0
    # the last pair: a document of all pads
    d[B - 1] = 0
    return q, d


def check_ids(q, d):
    """the edge patterns the tests rely on"""
    B, Q = q.shape
    L = d.shape[1]
    P = L // 100
    assert d[0, 0] == q[0, 0] and d[0, 99] == q[0, Q - 1] and d[0, P * 100 - 1] == q[0, 0]          # matches in columns 0 and 99
    assert q[1, Q - 1] == 0 and (d[1, L // 2:] == 0).all() and (d[1, : L // 2] != 0).all()           # both-pad mask; pad against real terms
    assert (q[3] == 0).all() and (d[3, 10:20] == 0).all() and (d[3, 20:] != 0).all()                 # an all-pad query
    assert (d[B - 1] == 0).all() and (q[B - 1] != 0).any()                                           # an all-pad document
    assert (d[2] == TINY_TOKEN).any() and (d[2] == q[2, 0]).any()
    if Q > 1:
        assert q[2, Q - 1] == q[2, 0] and (q[2] == TINY_TOKEN).sum() == (1 if Q > 2 else 2)          # a repeated term; the tiny row
    if L % 100:
        assert (d[:B - 1, P * 100:] != 0).any()                                                      # a live tail that must be ignored


def inputs(name):
    """make_ids for a fixture (its own stream, seed + 2000); the gradient case draws a second set of documents as the negatives"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"] + 2000)
    q, d = make_ids(rs, c["B"], c["Q"], c["L"])
    if name == "hint_grad":
        neg = rs.randint(0, V, size=d.shape).astype(np.int64)
        neg[:, :c["Q"]] = q
        return q, d, neg
    return q, d


# every (Q, L) of the sweep of the device tests: query lengths on both sides of the front end's group of four and up to the limit,
# documents of one window, of two and a half, and of the reference's default eight
SWEEP = tuple((Q, L) for Q in (1, 3, 4, 5, 8, 32) for L in (100, 250, 800))


def sweep_case(Q, L):
    """(config, extractor, weights, query ids [3, Q], document ids [3, L]) of a sweep point, all from one stream seeded by (Q, L):
    random ids with pads on both sides - a document in range, one with a padded tail against a padded query term, one of pads"""
    rs = np.random.RandomState(1000 * Q + L)
    kmax = min(2 * (L // 100), 3)
    ex = SimpleNamespace(embeddings=embeddings("hint_small"), pad=0, config={"maxqlen": Q, "maxdoclen": L})
    cfg = dict(DEFAULTS, kmax=kmax)
    w = make_weights(rs, D, kmax)
    q = rs.randint(1, V, size=(3, Q)).astype(np.int64)
    d = rs.randint(0, V, size=(3, L)).astype(np.int64)
    d[:, :Q] = np.where(rs.rand(3, Q) < 0.5, q, d[:, :Q])
    q[1, Q - 1] = 0
    d[1, L // 2:] = 0
    d[2] = 0
    return cfg, ex, w, q, d


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
