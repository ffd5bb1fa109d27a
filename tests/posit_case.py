"""POSITDRMM fixtures (tests/golden/posit_*.npz, made by tests/golden/make_golden_posit.py from the reference POSITDRMM_class): the
numpy-seeded embedding tables, weights, ids, idf and searcher scores both sides load, and the loader the tests use.  The .npz files hold
only ids, configuration and reference outputs."""
import os
from types import SimpleNamespace

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V, D = 64, 24
TINY_TOKEN = 5      # a token whose embedding row has norm ~1e-7: the wrong epsilon (or one in the context cosine) changes its cosines

# each the smallest shape at which a distinct mistake shows (the table of DESIGN §3.9)
CASES = {
    "posit_small": dict(Q=3, L=7, B=5, seed=71),       # every pad path of the layouts: trailing document pads, a padded query term, an all-pad query
    "posit_five": dict(Q=1, L=5, B=5, seed=72),        # top-5 equals the whole row; a query of one step
    "posit_ties": dict(Q=4, L=12, B=5, seed=73),       # repeated terms: equal cosines, match counts below / at / above 5, a query bigram in the document
    "posit_dim300": dict(Q=4, L=40, B=17, seed=74, D=300),   # the real width (pads to 320); a second, ragged sequence tile
    "posit_long": dict(Q=4, L=800, B=5, seed=75),      # error growth over 800 steps, both directions
    "posit_grad": dict(Q=3, L=9, B=5, seed=76),        # forward(pos, neg) and the gradients of a fixed linear loss
}
SCORE_CASES = ("posit_small", "posit_five", "posit_ties", "posit_dim300", "posit_long")
CONTEXT_CASES = ("posit_small", "posit_five", "posit_ties", "posit_dim300")     # the context tensors are recorded only where they are small
CONTEXT_PAIRS = {"posit_dim300": (0, 4, 16)}     # ... and at the real width for three pairs only, one of them in the second sequence tile


def context_pairs(name):
    return list(CONTEXT_PAIRS.get(name, range(CASES[name]["B"])))


def dim(name):
    return CASES[name].get("D", D)


def make_embeddings(rs, v=V, d=D):
    """[v, d] fp32 at scale 0.5; row 0 (the pad) all zeros, row TINY_TOKEN of norm ~1e-7"""
    emb = (rs.randn(v, d) * 0.5).astype(np.float32)
    emb[0] = 0.0
    emb[TINY_TOKEN] = (emb[TINY_TOKEN] / np.linalg.norm(emb[TINY_TOKEN]) * 1e-7).astype(np.float32)
    return emb


def embeddings(name):
    return make_embeddings(np.random.RandomState(CASES[name]["seed"]), d=dim(name))


def extractor(name):
    c = CASES[name]
    return SimpleNamespace(embeddings=embeddings(name), pad=0, config={"maxqlen": c["Q"], "maxdoclen": c["L"]})


def make_weights(rs, d):
    """state_dict entries (numpy fp32) of a model, all but posit1.embedding.weight.  Wider than PyTorch's default init (uniform in
    +- 1 / sqrt(d)): the gates leave their linear range and the scores of a case spread over many error bounds."""

    def n(*shape, s):
        return (rs.randn(*shape) * s).astype(np.float32)

    w = {}
    for layer in (0, 1):
        for rev in ("", "_reverse"):
            k = d * (layer + 1)
            w[f"posit1.encoding_layer.weight_ih_l{layer}{rev}"] = n(4 * d, k, s=1.5 / k ** 0.5)
            w[f"posit1.encoding_layer.weight_hh_l{layer}{rev}"] = n(4 * d, d, s=1.5 / d ** 0.5)
            w[f"posit1.encoding_layer.bias_ih_l{layer}{rev}"] = n(4 * d, s=0.3)
            w[f"posit1.encoding_layer.bias_hh_l{layer}{rev}"] = n(4 * d, s=0.3)
    w["posit1.Q1.weight"], w["posit1.Q1.bias"] = n(1, 6, s=1.0), n(1, s=0.2)
    w["posit1.Wg.weight"], w["posit1.Wg.bias"] = n(1, 5, s=1.0), n(1, s=0.2)
    return w


def weights(name):
    """make_weights for a fixture (its own stream, seed + 1000)"""
    return make_weights(np.random.RandomState(CASES[name]["seed"] + 1000), dim(name))


def make_ids(rs, B, Q, L, v=V):
    """int64 query ids [B, Q] and document ids [B, L] (B >= 5; every document keeps at least 2 terms) with the patterns check_ids asserts"""
    assert B >= 5 and L >= 5, (B, L)
    q = rs.randint(1, v, size=(B, Q)).astype(np.int64)
    d = rs.randint(1, v, size=(B, L)).astype(np.int64)
    q[q == TINY_TOKEN] = TINY_TOKEN + 1
    # pair 0: exact matches at both ends of the document; with L >= 12 the first query term 3 times in all
    d[0, 0], d[0, L - 1] = q[0, 0], q[0, Q - 1]
    if L >= 12:
        d[0][d[0] == q[0, 0]] = q[0, 0] % (v - 1) + 1           # (no chance occurrences: the counts below are exact)
        d[0, 0], d[0, 4], d[0, 6] = q[0, 0], q[0, 0], q[0, 0]
    # pair 1: a padded query term against a document with trailing pads; with L >= 12 the first query term exactly 5 times
    if Q > 1:
        q[1, Q - 1] = 0
    d[1, L - 2:] = 0
    if L >= 12:
        d[1][d[1] == q[1, 0]] = q[1, 0] % (v - 1) + 1
        d[1, 0:5] = q[1, 0]
    # pair 2: the tiny-norm row in the document (and in the query if Q > 2), a query term repeated in the query; with L >= 12 a term 7 times
    d[2, 1] = TINY_TOKEN
    if Q > 2:
        q[2, 1] = TINY_TOKEN
    if Q > 1:
        q[2, Q - 1] = q[2, 0]
    if L >= 12:
        d[2, 2:9] = q[2, 0]
    # pair 3: a query of all pads (Q > 1) against a document with a pad inside, which its bigrams span
    if Q > 1:
        q[3] = 0
    d[3, 2] = 0
    # pair 4: a query bigram in the document (Q > 1), once plainly and once across a removed pad; all but two terms pads
    if Q > 1:
        d[4, 0:2] = q[4, 0:2]
        d[4, 2:] = 0
        if L >= 12:
            d[4, 5], d[4, 7] = q[4, 0], q[4, 1]
    else:
        d[4, 2:] = 0
    return q, d


def check_ids(q, d):
    """the edge patterns the tests rely on"""
    B, Q = q.shape
    L = d.shape[1]
    assert ((d != 0).sum(1) >= 2).all()
    assert d[0, 0] == q[0, 0] and d[0, L - 1] == q[0, Q - 1]
    assert (d[1, L - 2:] == 0).all() and (d[1, :L - 2] != 0).all()
    assert (d[2] == TINY_TOKEN).any() and d[3, 2] == 0 and (d[3, 3:] != 0).all()
    if Q > 1:
        assert q[1, Q - 1] == 0 and (q[3] == 0).all() and q[2, Q - 1] == q[2, 0]
        assert (d[4, 0:2] == q[4, 0:2]).all() and (q[4, 0:2] != 0).all()
    if L >= 12:
        assert (d[0] == q[0, 0]).sum() in (3, 4) and (d[1] == q[1, 0]).sum() == 5 and (d[2] == q[2, 0]).sum() >= 7
        assert d[4, 5] == q[4, 0] and d[4, 6] == 0 and d[4, 7] == q[4, 1]


def inputs(name):
    """(query ids, document ids, idf [B, Q], searcher scores [B]) of a fixture (its own stream, seed + 2000); the gradient case draws a
    second set of documents and searcher scores as the negatives: (q, d, idf, bm25, neg, neg_bm25)"""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"] + 2000)
    q, d = make_ids(rs, c["B"], c["Q"], c["L"])
    idf = (rs.rand(c["B"], c["Q"]) * 3.0).astype(np.float32)
    bm25 = (rs.rand(c["B"]) * 2.0).astype(np.float32)
    if name == "posit_grad":
        neg = rs.randint(1, V, size=d.shape).astype(np.int64)
        neg[:, :c["Q"]] = q
        neg[1, c["L"] - 3:] = 0
        return q, d, idf, bm25, neg, (rs.rand(c["B"]) * 2.0).astype(np.float32)
    return q, d, idf, bm25


def load(name):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return {k: z[k] for k in z.files}


def build(name, plugin_cls):
    """(plugin, model) with the fixture's weights, on the CPU"""
    return build_from(extractor(name), weights(name), plugin_cls)


def build_from(ex, w, plugin_cls):
    import torch

    r = plugin_cls({}, ex)
    m = r.build_model()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    return r, m


def loop_stats(query_idf, query, doc, pad=0):
    """get_exact_match_stats spelled out pair by pair, query word by query word and bigram by bigram in plain Python (integer counts,
    Python-float divisions stored to fp32, the idf sum in fp32 in query order): what the vectorised and the device forms must equal"""
    out = np.zeros((doc.shape[0], 3), dtype=np.float32)
    for b in range(doc.shape[0]):
        cleaned = [int(t) for t in doc[b] if t != pad]
        matches, widf = 0, np.float32(0.0)
        for i, word in enumerate(query[b]):
            n = sum(1 for t in cleaned if t == word)
            matches += n
            widf = np.float32(widf + np.float32(np.float32(n) * np.float32(query_idf[b, i])))
        pairs = list(zip(cleaned[:-1], cleaned[1:]))
        bigrams = sum(1 for i in range(len(query[b]) - 1) for p in pairs if p == (int(query[b, i]), int(query[b, i + 1])))
        out[b] = (np.float32(matches / len(cleaned)), np.float32(widf / np.float32(len(cleaned))), np.float32(bigrams / len(pairs)))
    return out


def reference_outputs(name):
    """the fixture's outputs per quantity, as the reference computed them in fp32: score [B], features [B, Q, 6] and, where recorded, the
    context tensors [pairs, S, 2 D] (its LSTM outputs plus the embedded rows per direction, the fp32 sum it forms itself)"""
    c = load(name)
    out = {"score": c["score"], "features": c["features"]}
    if "lstm_doc" in c:
        emb, pairs = embeddings(name), context_pairs(name)
        for key, ids in (("query_context", c["query"]), ("doc_context", c["posdoc"])):
            x = emb[ids[pairs]]
            out[key] = c["lstm_query" if key == "query_context" else "lstm_doc"] + np.concatenate([x, x], axis=2)
    return out


_yardsticks = {}


def yardstick(name, plugin_cls):
    """(float64 restatement per quantity, e_ref per quantity = max |reference fp32 - float64|) of a fixture - computed once, shared, left
    alone.  The context tensors are those of context_pairs(name)."""
    import torch

    if name not in _yardsticks:
        c = load(name)
        m = build(name, plugin_cls)[1].eval()
        with torch.no_grad():
            score, det = m._forward_aten(torch.from_numpy(c["posdoc"]), torch.from_numpy(c["query"]), torch.from_numpy(c["query_idf"]),
                                         torch.from_numpy(c["extras"]), dtype=torch.float64, return_details=True)
        f64 = {"score": score.numpy(), "features": det["features"].numpy()}
        pairs = context_pairs(name)
        f64["query_context"], f64["doc_context"] = det["query_context"].numpy()[pairs], det["doc_context"].numpy()[pairs]
        ref = reference_outputs(name)
        _yardsticks[name] = (f64, {k: float(np.abs(ref[k] - f64[k]).max()) for k in ref})
    return _yardsticks[name]


def bound(e_ref, scale):
    """the tolerance of a quantity: max(4 e_ref, 16 fp32 ulp of its largest magnitude in the case)"""
    return max(4.0 * e_ref, 16.0 * float(np.spacing(np.float32(scale))))
