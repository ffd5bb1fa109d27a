"""Birch fixtures (tests/golden/birch_*.npz, made by tests/golden/make_golden_birch.py from the reference Birch_Class): the loader, the
seeded `combine` weights, and a float64 numpy restatement of what the reference does around its encoder (birch.py:92-109: which passages
are encoded, in which sub-batch, cut where; :121-125, 81-82: fill, top-k, combine).  Encoder weights are
capreolus_amd.synthetic.random_bert_weights by the fixture's seed, the next-sentence head its classifier scaled by `head_scale`."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("birch_mini", "birch_hidden", "birch_mixed", "birch_wide")
GRAD_CASES = ("birch_mini", "birch_hidden")
# the end-to-end bound on a passage logit: this factor times the reference's own autocast error + 1e-4 (test_bert_maxp_end_to_end's rule)
E2E_FACTOR = {"fp16": 1.25, "bf16": 1.5}
SIGMOID_D1_MAX = 0.25                      # max |sigma'|
SIGMOID_D2_MAX = 1.0 / (6.0 * 3.0 ** 0.5)  # max |sigma''| = 1 / (6 sqrt 3)


def plan_restated(mask, seg, subbatch, truncate):
    """birch.py:92-109 on int arrays [B, P, S] -> dict(rows: the encoded (b, p) in the order the reference encodes them, cut: per encoded
    row the last position its sub-batch keeps, doc_first [B + 1], enc_mask [n_enc, S]: the rows' masks, cleared behind the cut)."""
    mask, seg = np.asarray(mask, dtype=np.int64), np.asarray(seg, dtype=np.int64)
    B, P, S = mask.shape
    rows, cuts, doc_first = [], [], [0]
    for b in range(B):
        sm = seg[b] + mask[b]
        valid = (sm == 2).sum(axis=1) > 2
        if not valid.any():
            valid[0] = True
        ps = [p for p in range(P) if valid[p]]
        for g0 in range(0, len(ps), subbatch):
            group = ps[g0:g0 + subbatch]
            cut = max(int(np.argmax(sm[p])) for p in group) if truncate == "reference" else S - 1     # (np.argmax: the first maximum)
            rows += [(b, p) for p in group]
            cuts += [cut] * len(group)
        doc_first.append(len(rows))
    enc_mask = np.stack([np.where(np.arange(S) <= c, mask[b, p], 0) for (b, p), c in zip(rows, cuts)]) if rows else np.zeros((0, S), np.int64)
    return dict(rows=rows, cut=np.array(cuts, dtype=np.int64), doc_first=np.array(doc_first, dtype=np.int64), enc_mask=enc_mask)


def combine_restated(top, combine):
    """combine (birch.py:41-47) in float64 on top-k rows [B, topk]; combine: state_dict names -> arrays"""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in combine.items()}
    top = np.asarray(top, dtype=np.float64)
    if "combine.weight" in w:
        return top @ w["combine.weight"].reshape(-1)
    h = np.maximum(top @ w["combine.0.weight"].T + w["combine.0.bias"], 0.0)
    return h @ w["combine.2.weight"].reshape(-1) + w["combine.2.bias"][0]


def head_restated(enc_logits, doc_first, P, topk, combine):
    """birch.py:121-125, 81-82 in float64: -> (scores [B], top-k values [B, topk] descending, passage scores [B, P]: the encoded logits,
    then their minimum)"""
    x = np.asarray(enc_logits, dtype=np.float64)
    B = len(doc_first) - 1
    ps = np.empty((B, P))
    for b in range(B):
        own = x[doc_first[b]:doc_first[b + 1]]
        ps[b, :len(own)] = own
        ps[b, len(own):] = own.min()
    top = -np.sort(-ps, axis=1)[:, :topk]
    return combine_restated(top, combine), top, ps


def score_bound(combine, logit_bound):
    """The bound on a document's score that follows from a bound on every passage logit: the minimum and the order statistics are
    1-Lipschitz in the sup norm, so every top-k value moves by at most logit_bound; combine then multiplies by ||w||_1 (hidden = 0) or by
    sum_j |w2_j| sum_i |W1_ji| (ReLU is 1-Lipschitz)."""
    w = {k: np.abs(np.asarray(v, dtype=np.float64)) for k, v in combine.items()}
    if "combine.weight" in w:
        return float(w["combine.weight"].sum()) * logit_bound
    return float(w["combine.2.weight"].reshape(-1) @ w["combine.0.weight"].sum(axis=1)) * logit_bound


def birch_combine_weights(seed, topk, hidden):
    """`combine` of a fixture under Birch_Class's state_dict names (torch fp32): the reference's 1 / topk for hidden = 0, seeded otherwise"""
    import torch

    if hidden == 0:
        return {"combine.weight": torch.ones(1, topk) / topk}
    g = torch.Generator().manual_seed(seed + 3000)
    n = lambda *shape, s: torch.randn(*shape, generator=g) * s
    return {"combine.0.weight": n(hidden, topk, s=0.7), "combine.0.bias": n(hidden, s=0.5), "combine.2.weight": n(1, hidden, s=0.5),
            "combine.2.bias": n(1, s=0.1)}


def birch_weights(seed, dims, head_scale):
    """(the reference Birch_Class.bert's state_dict: ``bert.*`` + ``cls.seq_relationship.*``) from synthetic.random_bert_weights"""
    from capreolus_amd import synthetic

    hidden, layers, heads, ffn, vocab, max_pos = dims
    w = synthetic.random_bert_weights(hidden, layers, heads, ffn, vocab, max_pos, seed=seed)
    out = {k: v for k, v in w.items() if k.startswith("bert.")}
    out["cls.seq_relationship.weight"] = w["classifier.weight"] * head_scale
    out["cls.seq_relationship.bias"] = w["classifier.bias"]
    return out


def load_birch_case(name):
    """(fixture dict, Birch_Class.bert state_dict, combine state_dict, geometry for the plugin's `pretrained`)"""
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    c = {k: z[k] for k in z.files}
    dims = [int(x) for x in c["dims"]]
    bert = birch_weights(int(c["weight_seed"]), dims, float(c["head_scale"]))
    combine = birch_combine_weights(int(c["weight_seed"]), int(c["topk"]), int(c["hidden"]))
    geom = dict(zip(("hidden", "layers", "heads", "ffn", "vocab", "max_pos"), dims))
    return c, bert, combine, geom


def grad_restated(top_pos, top_neg, combine):
    """Gradients of pair_softmax_loss (reference reranker/common.py:96-98: mean(1 - softmax([pos, neg])[0]) = mean(1 - sigma(pos - neg)))
    with respect to combine's parameters, in float64, from the top-k rows of the positive and the negative documents.
    -> (grads by state_dict name, x: per parameter the per-pair derivative of (pos score - neg score) [B, ...], d: pos - neg scores)"""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in combine.items()}
    tp, tn = np.asarray(top_pos, dtype=np.float64), np.asarray(top_neg, dtype=np.float64)
    B = tp.shape[0]
    d = combine_restated(tp, combine) - combine_restated(tn, combine)
    sig = 1.0 / (1.0 + np.exp(-d))
    g = -sig * (1.0 - sig) / B                               # d loss / d (pos - neg)
    if "combine.weight" in w:
        x = {"combine.weight": (tp - tn)[:, None, :]}
    else:
        W1, b1, w2 = w["combine.0.weight"], w["combine.0.bias"], w["combine.2.weight"].reshape(-1)
        ap, an = tp @ W1.T + b1, tn @ W1.T + b1
        dp, dn = (ap > 0).astype(np.float64), (an > 0).astype(np.float64)
        x = {"combine.2.weight": (dp * ap - dn * an)[:, None, :], "combine.2.bias": np.zeros((B, 1)),
             "combine.0.bias": w2 * (dp - dn), "combine.0.weight": (w2 * dp)[:, :, None] * tp[:, None, :] - (w2 * dn)[:, :, None] * tn[:, None, :]}
    grads = {k: np.tensordot(g, v, axes=(0, 0)) for k, v in x.items()}
    return grads, x, d


def grad_bound(top_pos, top_neg, combine, eps):
    """Bounds on the error of grad_restated's gradients when every top-k value is off by at most eps and no hidden unit changes sides
    (relu_margin_ok).  With x = d (pos - neg score) / d theta per pair and g = -sigma'(d) / B:  grad = sum_b g_b x_b, so
    |delta grad| <= sum_b |delta g_b| |x_b| + |g_b'| |delta x_b| with |delta g_b| <= max|sigma''| |delta d_b| / B, |delta d_b| <= 2 L eps
    (score_bound: L eps per document), |g_b'| <= max|sigma'| / B, and |delta x_b| from the formulas of x: 2 eps for combine.weight;
    (D+ + D-) ||W1_j||_1 eps for combine.2.weight; 0 for the biases; |w2_j| (D+ + D-) eps for combine.0.weight."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in combine.items()}
    tp, tn = np.asarray(top_pos, dtype=np.float64), np.asarray(top_neg, dtype=np.float64)
    B = tp.shape[0]
    _, x, _ = grad_restated(tp, tn, combine)
    L = score_bound(combine, 1.0)
    if "combine.weight" in w:
        dx = {"combine.weight": np.full_like(x["combine.weight"], 2.0 * eps)}
    else:
        W1, b1, w2 = w["combine.0.weight"], w["combine.0.bias"], w["combine.2.weight"].reshape(-1)
        n = ((tp @ W1.T + b1 > 0).astype(np.float64) + (tn @ W1.T + b1 > 0))          # [B, hidden]: D+ + D-
        dx = {"combine.2.weight": (n * np.abs(W1).sum(axis=1) * eps)[:, None, :], "combine.2.bias": np.zeros((B, 1)),
              "combine.0.bias": np.zeros_like(n), "combine.0.weight": (np.abs(w2) * n)[:, :, None] * np.full((1, 1, tp.shape[1]), eps)}
    return {k: (SIGMOID_D2_MAX * 2.0 * L * eps * np.abs(x[k]) + SIGMOID_D1_MAX * dx[k]).sum(axis=0) / B for k in x}


def relu_margin_ok(top_pos, top_neg, combine, eps):
    """no hidden pre-activation lies within what eps can move it by (||W1_j||_1 eps) of the ReLU's kink: the premise of grad_bound"""
    if "combine.weight" in combine:
        return True
    W1, b1 = (np.asarray(combine[k], dtype=np.float64) for k in ("combine.0.weight", "combine.0.bias"))
    a = np.concatenate([np.asarray(t, dtype=np.float64) @ W1.T + b1 for t in (top_pos, top_neg)])
    return bool((np.abs(a) > np.abs(W1).sum(axis=1) * eps).all())
