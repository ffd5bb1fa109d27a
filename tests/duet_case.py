"""DUET fixtures (tests/golden/duet_*.npz, made by tests/golden/make_golden_duet.py from the reference DUET_class): the numpy-seeded
embedding tables, weights, ids and idf both sides load, a float64 restatement in numpy, and the loader the tests use.  The .npz files hold
only ids, configuration, state_dict names and shapes, and reference outputs."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V, D, Q, POOL = 64, 24, 4, 100

# each the smallest shape at which a distinct mistake shows: (default) the reference's defaults at dim 24: three tiles of pooled positions;
# (min) the smallest geometry the reference runs: two pooled positions, two filters, one hidden unit; (tanh_noidf) the other activation and
# the local model without idf; (dim300) rows of 1200 bytes: ten pieces of 32 floats, the last one short; (padrow) the table's row 0 is not
# zero: pads are embedded like any term; (grad) the gradient fixture of the training restatement (no dropout: the gradients are fixed)
CASES = {
    "duet_default": dict(L=800, B=6, seed=81, config={}),
    "duet_min": dict(L=103, B=6, seed=82, config={"nfilters": 2, "lmhidden": 1, "nhidden": 2}),
    "duet_tanh_noidf": dict(L=230, B=6, seed=83, config={"activation": "tanh", "idfweight": False, "nhidden": 129}),
    "duet_dim300": dict(L=250, B=6, seed=84, D=300, config={"nfilters": 3, "nhidden": 149}),
    "duet_padrow": dict(L=210, B=6, seed=85, config={"nfilters": 4, "nhidden": 109}, padrow=True),
    "duet_grad": dict(L=130, B=6, seed=86, config={"nfilters": 3, "lmhidden": 5, "nhidden": 29, "dropoutrate": 0.0}),
}
SCORE_CASES = tuple(n for n in CASES if n != "duet_grad")
DEFAULTS = {"nfilters": 10, "lmhidden": 30, "nhidden": 699, "idfweight": True, "dropoutrate": 0.5, "activation": "relu"}
OUTPUTS = ("score", "lm", "dm", "qvec", "pooled")


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


def make_extractor(emb, L):
    return SimpleNamespace(embeddings=emb, pad=0, config={"maxqlen": Q, "maxdoclen": L})


def extractor(name):
    return make_extractor(embeddings(name), CASES[name]["L"])


def make_weights(rs, cfg, L, dim):
    """state_dict entries (numpy fp32) of a model, all but dm.embedding.weight.  Wide: every layer's output has a spread of about one
    (scale 1.5 / sqrt(fan-in); the local convolution 0.5 per matching position) and the biases are small, so that neither activation
    flattens a case and its scores spread over many error bounds"""
    H, M, N = cfg["nfilters"], cfg["lmhidden"], cfg["nhidden"]

    def wide(*shape, fan):
        return (rs.randn(*shape) * (1.5 / np.sqrt(fan))).astype(np.float32)

    def small(n):
        return (rs.randn(n) * 0.1).astype(np.float32)

    return {"lm.conv.0.weight": (rs.randn(H, 1, 1, L) * 0.5).astype(np.float32), "lm.conv.0.bias": small(H),
            "lm.ffw.0.weight": wide(M, Q * H, fan=Q * H), "lm.ffw.0.bias": small(M),
            "lm.ffw.3.weight": wide(1, M, fan=M), "lm.ffw.3.bias": small(1),
            "dm.q_conv.0.weight": wide(H, 1, 3, dim, fan=0.25 * 3 * dim), "dm.q_conv.0.bias": small(H),
            "dm.q_ffw.0.weight": wide(H, H, fan=H), "dm.q_ffw.0.bias": small(H),
            "dm.d_conv1.0.weight": wide(H, 1, 3, dim, fan=0.25 * 3 * dim), "dm.d_conv1.0.bias": small(H),
            "dm.d_conv2.0.weight": wide(H, 1, H, 1, fan=H), "dm.d_conv2.0.bias": small(H),
            "dm.ffw_1.0.weight": wide(1, N, fan=N), "dm.ffw_1.0.bias": small(1),
            "dm.ffw_2.1.weight": wide(1, H, fan=H), "dm.ffw_2.1.bias": small(1)}


def weights(name):
    """make_weights for a fixture (its own stream, seed + 1000)"""
    c = CASES[name]
    return make_weights(np.random.RandomState(c["seed"] + 1000), config(name), c["L"], c.get("D", D))


SINGLE = 2          # the row of make_ids whose document has one term


def single_position(L):
    return L // 3


def make_ids(rs, B, L, v=V):
    """int64 query ids [B, 4], document ids [B, L], fp32 idf [B, 4] (B >= 6; every idf > 0, the pads' too).  Pair 0 repeats a query term
    at positions 0 and L - 1, the ends of the local weight row; pair 1 has a padded tail and a pad in its query: pad-pad matches; pair 2's
    document has one term, at single_position(L); pair 3 is a query of pads against a document without one; pair 4 has a short padded
    tail; pair 5 is a document of pads"""
    assert B >= 6, B
    q = rs.randint(1, v, size=(B, Q)).astype(np.int64)
    d = rs.randint(1, v, size=(B, L)).astype(np.int64)
    idf = rs.uniform(0.5, 3.0, size=(B, Q)).astype(np.float32)
    d[0, 0] = d[0, L - 1] = q[0, 1]
    d[1, (L + 1) // 2:] = 0
    q[1, 3] = 0
    d[SINGLE] = 0
    d[SINGLE, single_position(L)] = rs.randint(1, v)
    q[3] = 0
    d[4, L - 7:] = 0
    d[5] = 0
    return q, d, idf


def check_ids(q, d, idf):
    """the edge patterns the tests rely on"""
    B, L = d.shape
    assert d[0, 0] == d[0, L - 1] == q[0, 1] != 0
    assert (d[1, (L + 1) // 2:] == 0).all() and (d[1, :(L + 1) // 2] != 0).all() and q[1, 3] == 0 and idf[1, 3] > 0
    assert np.count_nonzero(d[SINGLE]) == 1 and d[SINGLE, single_position(L)] != 0
    assert (q[3] == 0).all() and (d[3] != 0).all() and (idf[3] > 0).all()
    assert (d[5] == 0).all() and (q[5] != 0).all()


def inputs(name):
    """make_ids for a fixture (its own stream, seed + 2000); the gradient case draws a second set of documents as the negatives"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"] + 2000)
    q, d, idf = make_ids(rs, c["B"], c["L"])
    if name == "duet_grad":
        return q, d, idf, rs.randint(0, V, size=d.shape).astype(np.int64)
    return q, d, idf


# every (L, nfilters, lmhidden, dim, activation) of the sweep of the device tests.
#   L: the smallest (two pooled positions), three, both sides of 128 and 192 (the local model walks the positions 64 at a time), 199 .. 203
#      (99 .. 102 pooled positions around the window of 100), 300, both sides of 256 and 512 pooled positions (L = 357 / 358, 613 / 614: the
#      document side runs in tiles of 256 pooled positions), 801;
#   nfilters: 2, 3, 10, 16, 32 - the 3 H projections of a term are held in 16, 16, 32, 48 and 96 accumulators, five instantiations of the
#      projection kernel; 21 and 26 are the remaining two (64 and 80);
#   lmhidden: 1, 30 and the limit 256;  dim: 23 (rows read as floats), 24, 50 (as floats: 50 % 4 != 0), 300, and the limit 512;
#   both activations.
SWEEP = tuple((L, 3, 30, 24, "relu") for L in (103, 104, 128, 129, 192, 193, 199, 200, 201, 202, 203, 300, 357, 358, 613, 614, 801)) + (
    (203, 2, 1, 23, "tanh"), (203, 10, 30, 24, "tanh"), (203, 16, 30, 50, "relu"), (203, 32, 30, 24, "tanh"), (203, 21, 30, 24, "relu"),
    (203, 26, 1, 23, "relu"), (230, 3, 256, 300, "tanh"), (104, 2, 256, 512, "relu"), (358, 10, 30, 300, "relu"), (358, 32, 1, 23, "relu"))
# the largest stated L and nfilters together (with the largest lmhidden): 32 tiles, the document kernel's 109 KiB of LDS
LIMITS = (8192, 32, 256, 24, "relu")


def sweep_case(L, H, M, dim, activation, B=3):
    """(config, extractor, weights, query ids [B, 4], document ids [B, L], idf [B, 4]) of a sweep point, all from one stream seeded by the
    point: a table whose row 0 is NOT zero; a random document with a query term at both ends, one with a padded tail under a query with a
    pad, one (B >= 3) with a single term; further documents are random"""
    rs = np.random.RandomState(((((L * 37 + H) * 263 + M) * 521 + dim) * 2 + (activation == "tanh")) % (1 << 32))
    cfg = dict(DEFAULTS, nfilters=H, lmhidden=M, nhidden=L - POOL - 1, activation=activation)
    ex = make_extractor(make_embeddings(rs, V, dim, padrow=True), L)
    w = make_weights(rs, cfg, L, dim)
    q = rs.randint(1, V, size=(B, Q)).astype(np.int64)
    d = rs.randint(1, V, size=(B, L)).astype(np.int64)
    idf = rs.uniform(0.5, 3.0, size=(B, Q)).astype(np.float32)
    d[0, 0] = d[0, L - 1] = q[0, 2]
    d[1, L // 2:] = 0
    q[1, 0] = 0
    if B > 2:
        d[2] = 0
        d[2, single_position(L)] = rs.randint(1, V)
    return cfg, ex, w, q, d, idf


def sweep_key(L, H, M, dim, activation):
    return f"{L}.{H}.{M}.{dim}.{activation}"


def restate(cfg, emb, w, q, d, idf):
    """DUET in float64, in numpy: {score [B], lm [B], dm [B], qvec [B, H], pooled [B, H, L - 101]}.  Ids are compared as they are in the
    local model; in the distributed model an id outside the table is a row of zeros"""
    def f(k):
        return np.asarray(w[k], dtype=np.float64)

    act = np.tanh if cfg["activation"] == "tanh" else (lambda x: np.maximum(x, 0.0))
    E = np.asarray(emb, dtype=np.float64)
    B, L = d.shape
    H = cfg["nfilters"]
    match = (q[:, :, None] == d[:, None, :]).astype(np.float64)
    if cfg["idfweight"]:
        match = match * np.asarray(idf, dtype=np.float64)[:, :, None]
    x = act(np.einsum("bqd,hd->bhq", match, f("lm.conv.0.weight").reshape(H, L)) + f("lm.conv.0.bias")[None, :, None])
    hid = act(x.reshape(B, -1) @ f("lm.ffw.0.weight").T + f("lm.ffw.0.bias"))
    lm = (hid @ f("lm.ffw.3.weight").T + f("lm.ffw.3.bias"))[:, 0]

    def rows(ids):
        ok = (ids >= 0) & (ids < E.shape[0])
        return np.where(ok[..., None], E[np.where(ok, ids, 0)], 0.0)

    def conv3(x, name):                                                                    # [B, T, dim] -> [B, H, T - 2]
        win = np.concatenate([x[:, :-2], x[:, 1:-1], x[:, 2:]], axis=2)
        return act(win @ f(name + ".weight").reshape(H, -1).T + f(name + ".bias")).transpose(0, 2, 1)

    qvec = conv3(rows(q), "dm.q_conv.0").max(axis=2) @ f("dm.q_ffw.0.weight").T + f("dm.q_ffw.0.bias")
    c = conv3(rows(d), "dm.d_conv1.0")
    pooled = np.lib.stride_tricks.sliding_window_view(c, POOL, axis=2).max(axis=-1)        # [B, H, L - 101]
    e = act(np.einsum("gh,bht->bgt", f("dm.d_conv2.0.weight").reshape(H, H), pooled) + f("dm.d_conv2.0.bias")[None, :, None])
    fo = act((qvec[:, :, None] * e) @ f("dm.ffw_1.0.weight")[0] + f("dm.ffw_1.0.bias")[0])
    dm = fo @ f("dm.ffw_2.1.weight")[0] + f("dm.ffw_2.1.bias")[0]
    return {"score": lm + dm, "lm": lm, "dm": dm, "qvec": qvec, "pooled": pooled}


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
