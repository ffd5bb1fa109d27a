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


# ---- the geometry sweep (tests/test_gpu_posit_geometry.py): points without a recorded reference ------------------------------------------
QUANTITIES = ("score", "features", "query_context", "doc_context")
_sweeps = {}


def sweep_ids(rs, B, Q, L, v=V):
    """int64 query ids [B, Q] and document ids [B, L] for B >= 2 and any Q <= 16, with the patterns check_sweep_ids asserts (pair i
    stands for pair i % B):
    pair 0: exact matches at both ends of the document (with L >= 12 the first query term three times);
    pair 1: a pad query term at Q - 1 - in the LAST group of four query terms - against a document with two trailing pads;
    pair 2: the tiny-norm row in the document (and in the query if Q > 2); the first query term again at the head of the last group of
            four (Q > 4; at Q - 1 below that) and, with Q > 8, term 3 again at 6; with L >= 12 that term seven times in the document;
    pair 3: a pad inside the document which a query bigram spans."""
    assert B >= 2 and L >= 5 and 1 <= Q <= 16, (B, Q, L)
    q = rs.randint(1, v, size=(B, Q)).astype(np.int64)
    d = rs.randint(1, v, size=(B, L)).astype(np.int64)
    q[q == TINY_TOKEN] = TINY_TOKEN + 1
    b0, b1, b2, b3 = (i % B for i in range(4))
    last = 4 * ((Q - 1) // 4)
    if Q > 1:
        q[b1, Q - 1] = 0
        q[b2, last if Q > 4 else Q - 1] = q[b2, 0]
    if Q > 2:
        q[b2, 1] = TINY_TOKEN
    if Q > 8:
        q[b2, 6] = q[b2, 3]
    d[b3, 2] = 0
    if Q > 1:
        d[b3, 1], d[b3, 3] = q[b3, 0], q[b3, 1]
    d[b0, 0], d[b0, L - 1] = q[b0, 0], q[b0, Q - 1]
    if L >= 12:
        d[b0, 4], d[b0, 6] = q[b0, 0], q[b0, 0]
    d[b2, 1] = TINY_TOKEN
    if L >= 12:
        d[b2, 2:9] = q[b2, 0]
    d[b1, L - 2:] = 0
    return q, d


def check_sweep_ids(q, d):
    """the patterns the sweep relies on"""
    B, Q = q.shape
    L = d.shape[1]
    b0, b1, b2, b3 = (i % B for i in range(4))
    last = 4 * ((Q - 1) // 4)
    assert ((d != 0).sum(1) >= 2).all()
    assert (d[b1, L - 2:] == 0).all() and d[b1, L - 3] != 0                 # a document with trailing pads
    assert (d[b2] == TINY_TOKEN).any() and d[b0, 0] == q[b0, 0] != 0 and d[b3, 2] == 0
    assert not (q[:, [i for i in range(Q) if i != 1]] == TINY_TOKEN).any()
    if Q > 1:
        assert q[b1, Q - 1] == 0 and (q[b1, :Q - 1] != 0).all()            # one pad query term, in the last group of four
        assert q[b2, 0] != 0 and (q[b2] == q[b2, 0]).sum() >= 2
    if Q > 4:
        assert Q - 1 >= last >= 4 and q[b2, last] == q[b2, 0]              # a term repeated across two groups of four
    if Q > 8:
        assert q[b2, 6] == q[b2, 3] != 0
    if L >= 12:
        assert (d[b2] == q[b2, 0]).sum() >= 7


def sweep_case(D, Q, L, B):
    """a point of the sweep, everything from one RandomState seeded by the point: the table (make_embeddings), the weights
    (make_weights), the ids (sweep_ids), idf [B, Q], extras [B, 4] (its last column doubles as the searcher's score, `bm25`).  Made
    once per point, shared, left alone."""
    key = (D, Q, L, B)
    if key not in _sweeps:
        rs = np.random.RandomState((D * 1000003 + Q * 10007 + L * 101 + B) % (1 << 31))
        ex = SimpleNamespace(embeddings=make_embeddings(rs, d=D), pad=0, config={})
        w = make_weights(rs, D)
        q, d = sweep_ids(rs, B, Q, L)
        idf, extras = (rs.rand(B, Q) * 3.0).astype(np.float32), (rs.rand(B, 4) * 2.0).astype(np.float32)
        _sweeps[key] = dict(point=key, ex=ex, w=w, query=q, posdoc=d, query_idf=idf, extras=extras, bm25=extras[:, 3].copy())
    return _sweeps[key]


def sweep_yardstick(case, plugin_cls):
    """(float64 restatement per quantity, e_ref per quantity = max |fp32 restatement - float64|) of a sweep_case (or a lane_case) - the
    fp32 restatement reproduces the reference bit for bit on every fixture (tests/test_posit_cpu.py).  Computed once per case."""
    import torch

    if "yardstick" not in case:
        host = build_from(case["ex"], case["w"], plugin_cls)[1].eval()
        t = [torch.from_numpy(case[k]) for k in ("posdoc", "query", "query_idf", "extras")]
        with torch.no_grad():
            s64, d64 = host._forward_aten(*t, dtype=torch.float64, return_details=True)
            s32, d32 = host._forward_aten(*t, return_details=True)
        f64 = {"score": s64.numpy(), **{k: d64[k].numpy() for k in QUANTITIES[1:]}}
        f32 = {"score": s32.numpy(), **{k: d32[k].numpy() for k in QUANTITIES[1:]}}
        case["yardstick"] = (f64, {k: float(np.abs(f32[k] - f64[k]).max()) for k in QUANTITIES})
    return case["yardstick"]


def matching_case():
    """(query ids [40, 16], document ids [40, 23], idf, searcher scores): ids from six tokens with pads anywhere (two leading document
    terms kept), so that every query term matches several times and bigrams are frequent - the idf sum has sixteen non-zero products"""
    rs = np.random.RandomState(16)
    q, d = rs.randint(0, 6, size=(40, 16)).astype(np.int64), rs.randint(0, 6, size=(40, 23)).astype(np.int64)
    d[:, :2] = rs.randint(1, 6, size=(40, 2))
    return q, d, (rs.rand(40, 16) * 3).astype(np.float32), rs.rand(40).astype(np.float32)


def fused_idf_stat(query_idf, query, doc, pad=0):
    """the second match statistic as a kernel gives it that fuses each product into the running sum (one rounding per term, where the
    reference rounds the product and the sum): what loop_stats' column 1 must NOT be confused with"""
    out = np.zeros(doc.shape[0], dtype=np.float32)
    for b in range(doc.shape[0]):
        cleaned = [t for t in doc[b] if t != pad]
        widf = np.float32(0.0)
        for i, word in enumerate(query[b]):
            widf = np.float32(float(sum(1 for t in cleaned if t == word)) * float(query_idf[b, i]) + float(widf))     # exact in float64
        out[b] = widf / np.float32(len(cleaned))
    return out


# ---- the top-5 of one lane -------------------------------------------------------------------------------------------------------------
LANE_POINT = (24, 4, 400, 3)
LANE_VARIANTS = ("ascending", "descending", "ties", "decoy")
LANE_SLOTS = 7 + 64 * np.arange(6)                     # six positions of lane 7 of the wave that pools the row
DECOY_TOP = np.array([3, 74, 148, 225, 306])           # lanes 3, 10, 20, 33, 50
DECOY_REST = 3 + 64 * np.arange(1, 6)                  # lane 3 again: behind its head, the 6th .. 10th largest of the row
_lanes = {}


def cosines(emb, qtok, toks):
    """M_cos of one query token against tokens, in float64 as the model forms it (1e-7 added to each norm)"""
    e = np.asarray(emb, dtype=np.float64)
    qv = e[qtok] / (np.linalg.norm(e[qtok]) + 1e-7)
    dv = e[toks] / (np.linalg.norm(e[toks], axis=-1, keepdims=True) + 1e-7)
    return dv @ qv


def lane_case(variant):
    """LANE_POINT with the document of pair 0 rebuilt around the table's ranking by cosine against q[0, 0] (rank 0 is that token
    itself): filled from rank 20 and below, then
    ascending   the six best at LANE_SLOTS in ascending order of cosine - every arrival is the lane's new maximum;
    descending  the same six in descending order - every arrival enters at the tail, the sixth is dropped;
    ties        the query token at all six - six equal maxima in one lane;
    decoy       the five best in five lanes (DECOY_TOP), the 6th .. 10th best all behind the first of them (DECOY_REST)."""
    if variant not in _lanes:
        base = sweep_case(*LANE_POINT)
        emb, qtok, L = base["ex"].embeddings, int(base["query"][0, 0]), LANE_POINT[2]
        order = np.argsort(-cosines(emb, qtok, np.arange(V)), kind="stable")
        assert order[0] == qtok
        d = base["posdoc"].copy()
        d[0] = np.random.RandomState(400 + LANE_VARIANTS.index(variant)).choice(order[20:], size=L)
        if variant == "ascending":
            d[0, LANE_SLOTS] = order[:6][::-1]
        elif variant == "descending":
            d[0, LANE_SLOTS] = order[:6]
        elif variant == "ties":
            d[0, LANE_SLOTS] = qtok
        else:
            d[0, DECOY_TOP], d[0, DECOY_REST] = order[:5], order[5:10]
        _lanes[variant] = dict({k: v for k, v in base.items() if k != "yardstick"}, posdoc=d, point=LANE_POINT + (variant,))
    return _lanes[variant]


def lane_row(case):
    """(the float64 cosine row of pair 0's first query term, its positions from the largest down - equal entries in order of position)"""
    row = cosines(case["ex"].embeddings, int(case["query"][0, 0]), case["posdoc"][0])
    return row, np.argsort(-row, kind="stable")


def check_lane(case, feature_bound):
    """What makes a lane variant a test of the per-lane top-5, on float64 alone.  ascending / descending / ties: the six largest of the
    row sit in ONE lane (positions congruent mod 64), and a fifth of the gap between the 5th and the 6th largest is more than 1000
    feature bounds - for `ties`, whose six largest are equal by construction, the gap is taken from them to the 7th largest.  A lane
    that kept four, or a pop in a wrong lane, then misses the mean of the top 5 by orders of magnitude.  decoy: the five largest in
    five lanes, the 6th .. 10th in the lane of the largest, the same margin between the 5th and the 6th."""
    variant = case["point"][-1]
    row, top = lane_row(case)
    v = row[top]
    print(f"\nlane {variant}: positions {top[:10].tolist()} values {np.round(v[:10], 4).tolist()} feature bound {feature_bound:.3g}")
    if variant == "decoy":
        assert len(set((top[:5] % 64).tolist())) == 5 and set((top[5:10] % 64).tolist()) == {int(top[0]) % 64}
        assert (v[4] - v[5]) / 5 > 1000 * feature_bound and v[9] > v[10]
        return
    assert len(set((top[:6] % 64).tolist())) == 1 and sorted(top[:6].tolist()) == LANE_SLOTS.tolist()
    if variant == "ties":
        assert v[0] == v[5]
    else:
        assert (v[4] - v[5]) / 5 > 1000 * feature_bound
        assert top[:6].tolist() == (LANE_SLOTS[::-1] if variant == "ascending" else LANE_SLOTS).tolist()
    assert (v[5] - v[6]) / 5 > 1000 * feature_bound


# ---- the chunks of steps (posit.hip: chunk_steps, carve) ----------------------------------------------------------------------------------
PROJ_BYTES = 512 << 20
# (D, Q, L of the base pairs, pairs in the one micro-batch) -> (T, the query side's chunks, the document side's chunks), rec_kernel<NB>
CHUNK_POINTS = {
    "three_chunks_gemm_tile_3": ((150, 4, 200, 1000), (87, [4], [87, 87, 26]), 3),
    "three_chunks_widest": ((300, 4, 120, 1000), (52, [4], [52, 52, 16]), 5),
    "chunked_query_one_step": ((24, 16, 5, 16400), (15, [15, 1], [5]), 1),
}
CHUNK_BASE_PAIRS = 5


def chunk_steps(n, D, Q, L):
    """positions per chunk of the recurrence for a micro-batch of n pairs, as posit.hip's chunk_steps"""
    Dp = (D + 63) // 64 * 64
    return int(min(max(PROJ_BYTES // (n * 8 * Dp * 4), 1), max(L, Q)))


def chunks(S, T):
    return [min(T, S - s0) for s0 in range(0, S, T)]


def workspace_bytes(n, D, Q, L, T):
    """posit.hip's carve for chunks of T steps: 4-byte cells, every buffer rounded up to 256 bytes"""
    Dp, S = (D + 63) // 64 * 64, max(L, Q)
    cells = (L * n * Dp, Q * n * Dp, S * n * 2 * Dp, L * n * 2 * Dp, Q * n * 2 * Dp, T * n * 8 * Dp, 2 * n * Dp, n * Q * L, n * Q * L, n * 4)
    return sum((4 * c + 255) // 256 * 256 for c in cells)
