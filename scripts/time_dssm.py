"""DSSM and CDSSM throughput at the reproduction's shapes, 1000 candidates of one query per call:

  CDSSM  4 query x 800 document terms, 300-d embeddings, defaults (windowsize 3, nkernel 3, nfilter 1): CDSSM.test (one tower launch per
         side + the pair kernel) and CDSSM.test_pairs (the query through its tower ONCE);
  DSSM   nvocab 400,001, nhiddens "56", documents of 800 tokens drawn Zipf 1.1: DSSM.test from Bags, DSSM.test from the dense
         [1000, 400001] matrix the reference reads (bags.from_dense included), and test_pairs from Bags.

Each is timed against the eager PyTorch restatement (_forward_aten, fp32, same GPU, same inputs) in the same process, the legs
interleaved round by round so that a neighbour's load on the machine falls on all of them: HIP events around `--iters` calls, the median
of `--rounds` rounds.  Run it under ONE time limit (`timeout -k 10 600 python scripts/time_dssm.py ...`).  Next to every time the
compulsory bytes are printed - what the kernels cannot avoid moving - and the time they take at the 6.3 TB/s this chip's HBM reaches:
  CDSSM  gathered: every embedding row the ids name, read once (rows x dim x 4); from HBM: the ids, the distinct rows, the outputs;
  DSSM   gathered: one padded row of W1^T per bag entry (nnz x 256 bytes) + the bags themselves; dense route: + the dense matrix once.

    python scripts/time_dssm.py [--candidates 1000] [--iters 5] [--rounds 5] [--no-eager] [--out profiles/dssm/time_dssm.json]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from capreolus_amd import bags  # noqa: E402
from capreolus_amd.reranker import CDSSM, DSSM  # noqa: E402

HBM_BYTES_PER_S = 6.3e12        # what a streaming copy reaches on this chip (8 TB/s on paper)


def timed(fn, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / iters / 1e3


def interleaved(legs, iters, rounds, warmup):
    """{name: median seconds per call}: every leg warmed up, then `rounds` rounds of every leg in turn"""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, iters))
    return {k: float(np.median(v)) for k, v in times.items()}, {k: [float(x) for x in v] for k, v in times.items()}


def cdssm_rows(a, dev):
    V, D, Q, L, B = 30000, 300, 4, 800, a.candidates
    rs = np.random.RandomState(0)
    emb = (rs.randn(V, D) * 0.5).astype(np.float32)
    emb[0] = 0
    q1 = torch.from_numpy(rs.randint(1, V, size=(1, Q))).to(dev)
    q = q1.repeat(B, 1)
    d = torch.from_numpy(rs.randint(1, V, size=(B, L)))
    lens = rs.randint(L // 4, L + 1, size=B)
    for i in range(B):                      # documents of the extractor's shape: real terms, then pads
        d[i, int(lens[i]):] = 0
    d = d.to(dev)
    torch.manual_seed(0)
    r = CDSSM({}, SimpleNamespace(embeddings=emb, pad=0, config={"maxqlen": Q, "maxdoclen": L}))
    m = r.build_model().to(dev).eval()
    batch = {"query": q, "posdoc": d}
    pq, pd = torch.zeros(B, dtype=torch.int32, device=dev), torch.arange(B, dtype=torch.int32, device=dev)
    legs = {"test": lambda: r.test(batch), "test_pairs": lambda: r.test_pairs(q1, d, pq, pd)}
    if not a.no_eager:
        legs["eager"] = lambda: m._forward_aten(d, q)
    with torch.no_grad():
        t, spread = interleaved(legs, a.iters, a.rounds, a.warmup)
        got = r.test(batch)
        same = bool(torch.equal(got, r.test_pairs(q1, d, pq, pd)))
        diff = None if a.no_eager else float((got - m._forward_aten(d, q)).abs().max())
    R = 3 * D - 3 + 1
    gathered = (B * L + B * Q) * D * 4
    distinct = int(torch.unique(torch.cat([d.reshape(-1), q.reshape(-1)])).numel())
    hbm = (B * L + B * Q) * 8 + distinct * D * 4 + (2 * B * R + B) * 4
    row = dict(model="CDSSM", candidates=B, Q=Q, L=L, D=D, vocab=V, call_s=t["test"], docs_per_s=B / t["test"], pairs_call_s=t["test_pairs"],
               pairs_equal_test=same, gathered_bytes=gathered, gathered_floor_s=gathered / HBM_BYTES_PER_S, hbm_bytes=hbm,
               hbm_floor_s=hbm / HBM_BYTES_PER_S, rounds=spread)
    if not a.no_eager:
        row.update(eager_s=t["eager"], speedup_over_eager=t["eager"] / t["test"], max_abs_diff_vs_eager=diff)
    return row


def dssm_rows(a, dev):
    nvocab, B, L = 400001, a.candidates, 800
    rs = np.random.RandomState(1)
    docs = [np.minimum(rs.zipf(1.1, size=L), nvocab) - 1 for _ in range(B)]
    q1 = bags.from_term_ids([rs.randint(0, nvocab, size=4)]).to(dev)
    qB = bags.from_term_ids([np.asarray(q1.idx.cpu())] * B).to(dev)
    d = bags.from_term_ids(docs).to(dev)
    nnz = int(d.idx.numel())
    torch.manual_seed(0)
    r = DSSM({}, SimpleNamespace(stoi=range(nvocab), pad=0))
    m = r.build_model().to(dev).eval()
    dense_q, dense_d = qB.to_dense(nvocab), d.to_dense(nvocab)
    pq, pd = torch.zeros(B, dtype=torch.int32, device=dev), torch.arange(B, dtype=torch.int32, device=dev)
    from_bags, from_dense = {"query": qB, "posdoc": d}, {"query": dense_q, "posdoc": dense_d}
    legs = {"bags": lambda: r.test(from_bags), "dense": lambda: r.test(from_dense), "test_pairs": lambda: r.test_pairs(q1, d, pq, pd)}
    if not a.no_eager:
        legs["eager"] = lambda: m._forward_aten(dense_d, dense_q)
    with torch.no_grad():
        t, spread = interleaved(legs, a.iters, a.rounds, a.warmup)
        got = r.test(from_bags)
        same = bool(torch.equal(got, r.test(from_dense)) and torch.equal(got, r.test_pairs(q1, d, pq, pd)))
        diff = None if a.no_eager else float((got - m._forward_aten(dense_d, dense_q)).abs().max())
    gathered = (nnz + int(qB.idx.numel())) * (256 + 8) + 2 * (B + 1) * 8 + (2 * B * 56 + B) * 4
    dense_bytes = gathered + 2 * B * nvocab * 4
    row = dict(model="DSSM", candidates=B, nvocab=nvocab, nhiddens="56", doc_tokens=L, doc_entries_mean=nnz / B, call_s=t["bags"],
               docs_per_s=B / t["bags"], dense_call_s=t["dense"], pairs_call_s=t["test_pairs"], routes_equal=same, gathered_bytes=gathered,
               gathered_floor_s=gathered / HBM_BYTES_PER_S, dense_bytes=dense_bytes, dense_floor_s=dense_bytes / HBM_BYTES_PER_S, rounds=spread)
    if not a.no_eager:
        row.update(eager_s=t["eager"], eager_bytes=2 * B * nvocab * 4 + nvocab * 56 * 4, speedup_over_eager=t["eager"] / t["bags"],
                   dense_speedup_over_eager=t["eager"] / t["dense"], max_abs_diff_vs_eager=diff)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_dssm.py measures on an MI355X; no GPU is visible (nothing is measured on the host)")
    dev = "cuda:0"
    rows = []
    for fn in (cdssm_rows, dssm_rows):
        row = fn(a, dev)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
