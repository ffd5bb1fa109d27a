"""The KNRM list pooling kernel (csrc/lists.hip: lists_knrm_pool_kernel) at the edges of its passes, with stale workspace beyond a
document's compact row, and with an exact-match kernel whose values are exactly zero over whole passes - capamd_knrm_forward_lists
against the per-pair capamd_knrm_forward on the same pairs, feature by feature, and against a float64 evaluation of KNRM.py's formula.

Features are read through a one-layer read-out with unit weights (score = feature k), one call per kernel.
  lists vs per-pair: 1e-6 relative on the features (tests/test_gpu_parity.py, test_lists_*: the same kernel values summed in another order).
  vs float64:        the formula in float64 over the C oracle's similarity matrix, relative to max(|feature|, 1); margin = twice the
                     per-pair kernel's worst error against the same reference on these inputs (F64_WORST_PER_PAIR below).
"""
import os
import re

import numpy as np
import pytest

import torch

from capreolus_amd import engine, synthetic
from oracle import cpu as oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LISTS_TOL = 1e-6       # tests/test_gpu_parity.py, test_lists_*
# Per-pair kernel against float64, relative to max(|feature|, 1): the worst figure over every case of this file, measured on an MI355X
# (each case prints its own): 1.4e-6, where the list route had 1.23e-6.  The margin for the list route is twice that.
F64_WORST_PER_PAIR = 1.4e-6
F64_MARGIN = 2 * F64_WORST_PER_PAIR
V, D, L = 1500, 300, 800
# a pass is TRIPS trips of W = 16 / 32 / 64 positions (3-4 / 2 / 1 real query terms): the library's own figure
_SRC = os.path.join(os.path.dirname(os.path.abspath(engine.__file__)), "csrc", "lists.hip")
TRIPS = int(re.search(r"^#define CAPAMD_POOL_TRIPS (\d+)", open(_SRC).read(), re.M).group(1))


def _t(a):
    return torch.as_tensor(a).to(DEV)


def pass_edge_counts():
    """real-term counts at the pass boundaries of every walk width: no pass, one partial pass, exactly k passes, one over"""
    c = {0, 1, 15, 16, 17, L}
    for w in (16, 32, 64):
        p = w * TRIPS
        for k in (1, 2, L // p):
            c |= {k * p - 1, k * p, k * p + 1}
    return sorted(x for x in c if 0 <= x <= L)


REF_MU = np.array([1.0, 0.9, 0.7, 0.5, 0.3, 0.1, -0.1, -0.3, -0.5, -0.7, -0.9], dtype=np.float32)
REF_SIGMA = np.array([0.001] + [0.1] * 10, dtype=np.float32)
BANKS = {
    "reference": (REF_MU, REF_SIGMA),
    "narrow_in_the_middle": (REF_MU[::-1].copy()[[1, 2, 3, 4, 10, 5, 6, 7, 8, 9, 0]], np.r_[[0.1] * 4, 0.001, [0.1] * 6].astype(np.float32)),
    "uniform": (REF_MU, np.full(11, 0.1, dtype=np.float32)),
    "twelve_uniform": (np.linspace(-0.9, 1.0, 12).astype(np.float32), np.full(12, 0.1, dtype=np.float32)),
}


def embeddings():
    emb = synthetic.make_embeddings(V, D, seed=21).copy()
    # rows with a controlled cosine to row 1 (the exact-match kernel is +0 in fp32 further than 0.0144 from 1): ids 2..5
    e0 = emb[1] / np.linalg.norm(emb[1])
    e1 = emb[6] - (emb[6] @ e0) * e0
    e1 /= np.linalg.norm(e1)
    for i, c in zip((2, 3, 4, 5), (1 - 0.0140, 1 - 0.0148, 1 - 0.0100, 1 - 0.0200)):
        emb[i] = (c * e0 + np.sqrt(1 - c * c) * e1) * 3.0
    return emb.astype(np.float32)


def docs_with_counts(rs, counts, lo=7):
    d = np.zeros((len(counts), L), dtype=np.int64)
    for i, c in enumerate(counts):
        d[i, :c] = rs.randint(lo, V, size=c)
    return d


def features(route, q, d, off, packed, mu, sigma, **kw):
    K = mu.shape[0]
    out = []
    for k in range(K):
        w1 = torch.zeros(K, device=DEV)
        w1[k] = 1.0
        b1 = torch.zeros(1, device=DEV)
        if route == "pairs":
            out.append(engine.knrm_forward(_t(q), _t(d), packed, V, D, _t(mu), _t(sigma), w1, b1).cpu().numpy())
        else:
            out.append(engine.knrm_forward_lists(off, packed, V, D, _t(mu), _t(sigma), w1, b1, **kw).cpu().numpy())
    return np.stack(out, axis=1).astype(np.float64)


def features_f64(q, d, emb, mu, sigma):
    """KNRM.py:39-55 in float64 over the C oracle's similarity matrix (OOV ids: 1 where equal, else 0 - common.py:155-158)"""
    sim, err = oracle.simmat(q, d, oracle.pack(emb), D)
    assert err == 0
    s = sim.astype(np.float64)                                                   # [B, Q, L]
    kv = np.exp(-((s[..., None] - mu.astype(np.float64)) ** 2) / (2.0 * sigma.astype(np.float64) ** 2))      # [B, Q, L, K]
    S = kv.sum(axis=2)                                                           # [B, Q, K]
    mask = (s.sum(axis=2) != 0.0)[..., None]
    return np.where(mask, np.log(S + 1e-6), 0.0).sum(axis=1)


def check(q, d, off, emb, bank, f64=True, **kw):
    mu, sigma = BANKS[bank]
    packed = engine.PackedEmbedding().get(_t(emb))
    pairs = features("pairs", q, d, off, packed, mu, sigma)
    if not kw:
        kw = {"query": _t(q), "doc": _t(d)}
    lists = features("lists", q, d, off, packed, mu, sigma, **kw)
    assert engine.status_word(DEV).t.item() == 0
    assert np.array_equal(lists == 0.0, pairs == 0.0)
    e_l = float((np.abs(lists - pairs) / np.where(pairs == 0.0, 1.0, np.abs(pairs))).max())
    print(f"lists vs per-pair {e_l:.3g}")
    if f64:
        want = features_f64(q, d, emb, mu, sigma)
        sc = np.maximum(np.abs(want), 1.0)
        e_p, e_w = float((np.abs(pairs - want) / sc).max()), float((np.abs(lists - want) / sc).max())
        print(f"per-pair vs float64 {e_p:.3g}   lists vs float64 {e_w:.3g}")
        assert e_w <= F64_MARGIN, (e_w, e_p)
    assert e_l <= LISTS_TOL, e_l
    return lists


def queries(rs, kind, n):
    q = np.zeros((n, 4), dtype=np.int64)
    if kind == "pads":
        return q
    if kind == "oov":
        q[:, :3] = [rs.randint(7, V), -7, rs.randint(7, V)]
        return q
    q[:, :kind] = rs.randint(7, V, size=kind)
    return q


@pytest.mark.parametrize("qkind", [1, 2, 3, 4, "oov", "pads"])
def test_pool_pipeline_edges(qkind):
    """One list of documents whose real-term counts are the pass boundaries of every walk width, per number of real query terms; a query
    with an OOV term a document matches; a query of pads only.  The workspace is filled with 0x7f bytes first: what the first pass reads
    of a compact row beyond its n are large positive ints and must never index the table (status word 0, same features)."""
    rs = np.random.RandomState(5)
    counts = pass_edge_counts()
    d = docs_with_counts(rs, counts)
    q = queries(rs, qkind, len(counts))
    if qkind == "oov":
        d[3, 0] = -7
        d[9, 20] = -7
        d[9, 700] = -9
    off = np.array([0, len(counts)], dtype=np.int64)
    engine._lists_pair_workspace(DEV, 1, V, len(counts), L, 4).fill_(0x7F)
    check(q, d, off, embeddings(), "reference")


@pytest.mark.parametrize("bank", ["reference", "narrow_in_the_middle", "uniform", "twelve_uniform"])
def test_pool_exact_zero_skip(bank):
    """Documents without an exact match; with exactly one position - in the last trip of the last pass - equal to the query term; with
    positions whose similarity is just inside / outside the distance from 1 at which the exact-match kernel (sigma 0.001) becomes +0 in
    fp32 (rows 2..5 of the table have a set cosine to row 1, the query term); under the reference bank, a bank whose narrow kernel is
    neither first nor last, and banks of sigma 0.1 throughout (K = 11, and K = 12: the kMaxK instantiation)."""
    rs = np.random.RandomState(9)
    full = 16 * TRIPS * 3      # three whole passes of the four-term walk
    counts = [full, full, 303, 303, 50, 50, 50, 50, 400]
    d = docs_with_counts(rs, counts)
    d[1, full - 1] = 1
    d[3, 302] = 1
    for i, r in zip((4, 5, 6, 7), (2, 3, 4, 5)):
        d[i, 49] = r
    d[8, 5], d[8, 399] = 2, 3
    emb = embeddings()
    for nreal in (1, 3):
        q = np.zeros((len(counts), 4), dtype=np.int64)
        q[:, 0] = 1
        q[:, 1:nreal] = rs.randint(7, V, size=nreal - 1)
        check(q, d, np.array([0, len(counts)], dtype=np.int64), emb, bank)


def test_pool_other_routes(monkeypatch):
    """Q = 8 (two blocks of four terms), the int32 resident store, and a call whose lists span two workspace chunks."""
    from capreolus_amd.feeder import CandidateStore

    rs = np.random.RandomState(13)
    counts = [0, 5, 16 * TRIPS, 16 * TRIPS + 1, 200, 64 * TRIPS + 1, 800, 303]
    d = docs_with_counts(rs, counts)
    emb = embeddings()
    off = np.array([0, 3, len(counts)], dtype=np.int64)
    q8 = np.zeros((len(counts), 8), dtype=np.int64)
    q8[:3, :6] = rs.randint(7, V, size=6)
    q8[3:, :5] = rs.randint(7, V, size=5)
    mu, sigma = BANKS["reference"]
    packed = engine.PackedEmbedding().get(_t(emb))
    check(q8, d, off, emb, "reference")
    q = q8[:, :4].copy()
    base = check(q, d, off, emb, "reference")
    store = CandidateStore(DEV)
    store.add_query("a", q[0], np.ones(4, dtype=np.float32))
    store.add_query("b", q[3], np.ones(4, dtype=np.float32))
    for j in range(len(counts)):
        store.add_doc(f"d{j}", d[j])
    store.finalize()
    pq = _t(np.array([0] * 3 + [1] * (len(counts) - 3), dtype=np.int32))
    pd = _t(np.arange(len(counts), dtype=np.int32))
    resident = features("lists", q, d, off, packed, mu, sigma, store=store, pair_q=pq, pair_d=pd)
    assert np.array_equal(resident, base)
    monkeypatch.setattr(engine, "LISTS_WORKSPACE_BUDGET", 1)      # room for one list in flight: two chunks
    engine.release_workspaces()
    try:
        chunked = features("lists", q, d, off, packed, mu, sigma, query=_t(q), doc=_t(d))
    finally:
        engine.release_workspaces()
    assert np.array_equal(chunked, base)
