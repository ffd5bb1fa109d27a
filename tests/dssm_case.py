"""DSSM fixtures (tests/golden/dssm_*.npz, made by tests/golden/make_golden_dssm.py from the reference DSSM_class): the numpy-seeded
weights and term rows both sides load, and the loader the tests use.  The .npz files hold only the bags in sparse form (never the dense
matrix), configuration and reference outputs."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# each the smallest shape at which a distinct mistake shows: (default) the reference's default width: query bags of at most 4 terms,
# documents of 200 tokens with repeats, an empty document bag, entries at index 0 and nvocab - 1; (two) a second layer, widths that
# are no multiple of 16, values that are no integers; (big) a vocabulary past 2^16 and one bag of 3,000 entries among tiny ones: long
# bags, the fixed partition over waves; (wide) four layers and a first width past 64: the kernel's instantiation for rows of more than
# one 64-float piece, and every later layer it has; (grad) the gradient fixture of the training restatement
CASES = {
    "dssm_default": dict(nvocab=500, B=6, doclen=200, seed=81, config={}),
    "dssm_two": dict(nvocab=500, B=6, doclen=200, seed=82, config={"nhiddens": "30 17"}, fractional=True),
    "dssm_big": dict(nvocab=70001, B=6, doclen=5, seed=83, config={}, big=3000),
    "dssm_grad": dict(nvocab=500, B=6, doclen=60, seed=84, config={"nhiddens": "30 17"}),
    "dssm_wide": dict(nvocab=500, B=6, doclen=200, seed=85, config={"nhiddens": "130 65 9 5"}),
}
SCORE_CASES = ("dssm_default", "dssm_two", "dssm_big", "dssm_wide")
DEFAULTS = {"nhiddens": "56"}


def config(name):
    return dict(DEFAULTS, **CASES[name]["config"])


def extractor(name):
    return make_extractor(CASES[name]["nvocab"])


def make_extractor(nvocab):
    return SimpleNamespace(stoi={i: i for i in range(nvocab)}, pad=0)


def make_weights(rs, nvocab, nhiddens):
    """state_dict entries (numpy fp32): ffw.linear<i>.weight / .bias.  The first layer at scale 0.1 against bags whose counts have a norm
    of 10 .. 20 puts its units at a scale of 1 .. 2 around small biases, so about half are cut by the ReLU, a different half per bag, and
    the cosines of a case spread over many error bounds"""
    widths = [nvocab] + [int(h) for h in str(nhiddens).split()]
    w = {}
    for i in range(len(widths) - 1):
        s = 0.1 if i == 0 else 1.0 / widths[i] ** 0.5
        w[f"ffw.linear{i}.weight"] = (rs.randn(widths[i + 1], widths[i]) * s).astype(np.float32)
        w[f"ffw.linear{i}.bias"] = (rs.randn(widths[i + 1]) * 0.1).astype(np.float32)
    return w


def weights(name):
    """make_weights for a fixture (its own stream, seed + 1000)"""
    return make_weights(np.random.RandomState(CASES[name]["seed"] + 1000), CASES[name]["nvocab"], config(name)["nhiddens"])


def make_rows(rs, B, nvocab, doclen, big=None):
    """(query term rows, document term rows): lists of B int64 arrays of any length (B >= 5).  Queries of 1 .. 4 terms; documents of
    `doclen` tokens drawn Zipf-like, so with repeats; document 0 holds index 0 and nvocab - 1, query 1 too; document 2 has `big` distinct
    terms if asked; query 3 repeats one term; the last document is empty"""
    assert B >= 5, B
    q = [rs.randint(0, nvocab, size=1 + b % 4).astype(np.int64) for b in range(B)]
    d = [((rs.zipf(1.3, size=doclen) - 1) * 7919 % nvocab).astype(np.int64) for b in range(B)]
    d[0][:2] = (0, nvocab - 1)
    q[1][0], q[1][-1] = 0, nvocab - 1
    q[3][:] = q[3][0]
    if big:
        d[2] = np.concatenate([rs.choice(nvocab, size=big, replace=False), d[2]]).astype(np.int64)
    d[B - 1] = np.zeros(0, dtype=np.int64)
    return q, d


def csr(rows, rs=None):
    """numpy (indptr int64, idx int32, val fp32) of unigram counts, each bag sorted by index; with rs the counts are scaled by factors in
    [0.25, 1.25): values that are no integers"""
    indptr, idx, val = [0], [], []
    for r in rows:
        ids, counts = np.unique(np.asarray(r, dtype=np.int64), return_counts=True)
        idx.append(ids.astype(np.int32))
        val.append(counts.astype(np.float32))
        indptr.append(indptr[-1] + len(ids))
    idx, val = np.concatenate(idx).astype(np.int32), np.concatenate(val).astype(np.float32)
    if rs is not None:
        val = (val * (0.25 + rs.rand(len(val)))).astype(np.float32)
    return np.asarray(indptr, dtype=np.int64), idx, val


def rows(name):
    """make_rows for a fixture (its own stream, seed + 2000); the gradient case draws a second set of documents as the negatives"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"] + 2000)
    q, d = make_rows(rs, c["B"], c["nvocab"], c["doclen"], c.get("big"))
    if name == "dssm_grad":
        return q, d, make_rows(rs, c["B"], c["nvocab"], c["doclen"])[1][::-1]
    return q, d


def inputs(name):
    """the bags of a fixture, one numpy (indptr, idx, val) per side of rows(name)"""
    rs = np.random.RandomState(CASES[name]["seed"] + 3000) if CASES[name].get("fractional") else None
    return tuple(csr(r, rs) for r in rows(name))


def check_bags(q, d, nvocab):
    """the edge patterns the tests rely on"""
    (qp, qi, _), (dp, di, _) = q, d
    assert (np.diff(qp) <= 4).all() and (np.diff(qp) >= 1).all()
    assert dp[-1] == dp[-2] and (np.diff(dp)[:-1] > 0).all()                     # the last document bag is empty
    assert di[dp[0]] == 0 and di[dp[1] - 1] == nvocab - 1                         # index 0 and nvocab - 1
    assert qi[qp[1]] == 0 and qi[qp[2] - 1] == nvocab - 1


def dense(bag, nvocab, dtype=np.float32):
    """the [N, nvocab] matrix of a numpy bag triple - what the reference reads"""
    indptr, idx, val = bag
    out = np.zeros((len(indptr) - 1, nvocab), dtype=dtype)
    for n in range(len(indptr) - 1):
        out[n, idx[indptr[n]:indptr[n + 1]]] = val[indptr[n]:indptr[n + 1]]
    return out


def load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return {k: z[k] for k in z.files}


def bags_of(c, side):
    """capreolus_amd.bags.Bags (CPU tensors) of a loaded fixture's side ("query", "posdoc", "negdoc")"""
    import torch

    from capreolus_amd.bags import Bags

    return Bags(*(torch.from_numpy(c[f"{side}.{k}"]) for k in ("indptr", "idx", "val")))


def build(name, plugin_cls):
    """(plugin, model) with the fixture's weights, on the CPU"""
    return build_from(config(name), extractor(name), weights(name), plugin_cls)


def build_from(cfg, ex, w, plugin_cls):
    import torch

    r = plugin_cls(cfg, ex)
    m = r.build_model()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return r, m
