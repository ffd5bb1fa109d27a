"""DeepTileBar at the reproduction's shape (1000 candidates of 4 query x 800 document terms, 300-d embeddings, 20 segments of about 40
tokens): the colouring call (capamd_deeptile_color), the model call (capamd_deeptile_forward), both in sequence (DeepTileBar.test_ids),
the eager PyTorch restatement of the model (DeepTileBar_class._forward_aten, fp32, on the same GPU and tiles) as the model's
denominator, and for a handful of documents the reference-style colouring on the host: a Python double loop over (query term, segment)
with one numpy norm per segment token.  HIP events after warm-up, median of three.

The colouring is reported against its compulsory bytes - every distinct embedding row the call touches once, plus the ids, offsets, idf
and tiles - and the share of the HBM peak those bytes give over its time.

    python scripts/time_deeptile.py [--candidates 1000] [--iters 100] [--host-docs 5] [--no-eager] [--out profiles/deeptile/time_deeptile.json]

Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_deeptile.py --no-eager --host-docs 0` (profiles/deeptile/).
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from capreolus_amd.reranker import DeepTileBar  # noqa: E402

HBM_PEAK = 8.0e12      # MI355X, bytes/s (specification)


def timed(fn, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / iters / 1e3


def host_colouring(q, d, seg, idf, emb):
    """one document the way the reference colours it: per (query term, segment) a generator of one numpy norm per token"""
    Q, P = len(q), len(seg) - 1
    out = np.zeros((Q, P, 3), dtype=np.float32)
    for i in range(Q):
        for p in range(P):
            toks = d[seg[p]:seg[p + 1]]
            if q[i] == 0 or not len(toks):
                continue
            tf = int((toks == q[i]).sum())
            sim = max(np.exp(-(np.linalg.norm(emb[t] - emb[q[i]]) ** 2) / 2) if t >= 0 else 0 for t in toks)
            out[i, p] = (tf, idf[i] if tf else 0, sim)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-docs", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev, V, D, Q, L, P, B = "cuda:0", 30000, 300, 4, 800, 20, a.candidates
    rs = np.random.RandomState(0)
    emb = (rs.randn(V, D) * (1.2 / D ** 0.5)).astype(np.float32)
    emb[0] = 0
    q = np.repeat(rs.randint(1, V, size=(1, Q)), B, axis=0)
    d = rs.randint(1, V, size=(B, L))
    d[rs.rand(B, L) < 0.02] = q[0, 0]                                      # the query's first term occurs now and then
    cuts = np.sort(rs.randint(20, L - 20, size=(B, P - 1)), axis=1)        # 20 segments of about 40 tokens that cover the row
    seg = np.concatenate([np.zeros((B, 1), int), cuts, np.full((B, 1), L)], axis=1).astype(np.int32)
    idf = np.repeat((rs.rand(1, Q) * 3 + 0.5).astype(np.float32), B, axis=0)
    torch.manual_seed(0)
    r = DeepTileBar({}, SimpleNamespace(embeddings=emb, config={"maxqlen": Q, "passagelen": P, "tfchannel": True}))
    m = r.build_model().to(dev).eval()
    batch = {"query": torch.from_numpy(q).to(dev), "posdoc": torch.from_numpy(d).to(dev), "posdoc_segments": torch.from_numpy(seg).to(dev),
             "query_idf": torch.from_numpy(idf).to(dev)}
    table = r._table(torch.device(dev))
    rows = len(np.unique(np.concatenate([d.reshape(-1), q.reshape(-1)])))
    compulsory = rows * D * 4 + d.size * 8 + q.size * 8 + seg.size * 4 + idf.size * 4 + B * Q * P * 3 * 4
    with torch.no_grad():
        tiles = r.color(batch, table)
        for _ in range(a.warmup):
            r.color(batch, table), r.test({"posdoc": tiles}), r.test_ids(batch, table)
        med = lambda fn, n=a.iters: float(np.median([timed(fn, n) for _ in range(3)]))       # noqa: E731
        t_color, t_model, t_both = med(lambda: r.color(batch, table)), med(lambda: r.test({"posdoc": tiles})), med(lambda: r.test_ids(batch, table))
        row = dict(candidates=B, Q=Q, L=L, D=D, P=P, color_s=t_color, model_s=t_model, both_s=t_both, docs_per_s=B / t_both,
                   distinct_rows=rows, color_compulsory_bytes=compulsory, color_gathered_bytes=int(d.size) * D * 4, hbm_peak=HBM_PEAK,
                   color_fraction_of_hbm_peak=compulsory / t_color / HBM_PEAK, color_gather_rate_bytes_per_s=int(d.size) * D * 4 / t_color)
        if not a.no_eager:
            ref = m._forward_aten(tiles)
            t_eager = med(lambda: m._forward_aten(tiles), max(1, a.iters // 10))
            got = r.test({"posdoc": tiles})
            row.update(eager_model_s=t_eager, model_speedup_over_eager=t_eager / t_model,
                       max_rel_diff_vs_eager=float(((got - ref).abs() / ref.abs().max()).max()))
        if a.host_docs:
            t0 = time.perf_counter()
            host = np.stack([host_colouring(q[i], d[i], seg[i], idf[i], emb) for i in range(a.host_docs)])
            t_host = (time.perf_counter() - t0) / a.host_docs
            row.update(host_colouring_s_per_doc=t_host, host_docs=a.host_docs, color_speedup_over_host_loop=t_host * B / t_color,
                       max_diff_vs_host_loop=float(np.abs(tiles[:a.host_docs].cpu().numpy() - host).max()))
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
