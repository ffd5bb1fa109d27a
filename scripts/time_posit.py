"""POSITDRMM throughput at the reproduction's shape (4 query x 800 document terms, 300-d embeddings, 1000 candidates per call, documents of
mixed real length): documents/s of POSITDRMM.test (capamd_posit_forward), the eager PyTorch restatement (POSITDRMM_class._forward_aten,
fp32, nn.LSTM through the library, on the same GPU and inputs, in chunks of documents) as the ratio's denominator, and the fraction of
the fp32 matrix peak on the model's own arithmetic (the LSTM's products at the real width, both sides).  HIP events after warm-up,
median of three.

    python scripts/time_posit.py [--candidates 1000] [--iters 3] [--no-eager] [--out profiles/posit/time_posit.json]

Stage shares: run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_posit.py --no-eager --iters 2` (profiles/posit/).
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

from capreolus_amd.reranker import POSITDRMM  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12      # MI355X, fp32 MFMA, dense


def timed(fn, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / iters / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--eager-chunk", type=int, default=250)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev, V, D, Q, L, B = "cuda:0", 30000, 300, 4, 800, a.candidates
    rs = np.random.RandomState(0)
    emb = (rs.randn(V, D) * 0.5).astype(np.float32)
    emb[0] = 0
    q = torch.from_numpy(rs.randint(1, V, size=(1, Q))).repeat(B, 1).to(dev)
    d = torch.from_numpy(rs.randint(1, V, size=(B, L))).to(dev)
    lens = rs.randint(L // 4, L + 1, size=B)
    for i in range(B):                      # documents of the extractor's shape: real terms, then pads
        d[i, int(lens[i]):] = 0
    idf = torch.from_numpy((rs.rand(1, Q) * 3).astype(np.float32)).repeat(B, 1).to(dev)
    torch.manual_seed(0)
    r = POSITDRMM({}, SimpleNamespace(embeddings=emb, pad=0, config={"maxqlen": Q, "maxdoclen": L}))
    m = r.build_model().to(dev).eval()
    r.searcher_scores = {"q": {i: float(v) for i, v in enumerate(rs.rand(B))}}
    batch = {"query": q, "posdoc": d, "query_idf": idf, "qid": ["q"] * B, "posdocid": list(range(B))}
    # the LSTM's multiply-adds per pair: per position, direction and layer 4 D gates x (input width + D)
    flop = 2.0 * (L + Q) * 2 * 4 * D * ((D + D) + (2 * D + D))
    with torch.no_grad():
        for _ in range(a.warmup):
            r.test(batch)
        t = float(np.median([timed(lambda: r.test(batch), a.iters) for _ in range(3)]))
        row = dict(candidates=B, Q=Q, L=L, D=D, call_s=t, docs_per_s=B / t, lstm_flop_per_doc=flop, fp32_matrix_peak=FP32_MATRIX_PEAK,
                   fraction_of_fp32_matrix_peak=flop * B / t / FP32_MATRIX_PEAK)
        if not a.no_eager:
            extras = torch.cat(r.get_exact_match_stats(idf, q, d) + (torch.tensor([r.searcher_scores["q"][i] for i in range(B)], device=dev).view(-1, 1),), 1)

            def eager():
                return torch.cat([m._forward_aten(d[i:i + a.eager_chunk], q[i:i + a.eager_chunk], idf[i:i + a.eager_chunk], extras[i:i + a.eager_chunk])
                                  for i in range(0, B, a.eager_chunk)])
            ref = eager()
            t_eager = float(np.median([timed(eager, 1) for _ in range(3)]))
            got = r.test(batch)
            row.update(eager_s=t_eager, eager_chunk=a.eager_chunk, eager_docs_per_s=B / t_eager, speedup_over_eager=t_eager / t,
                       max_rel_diff_vs_eager=float(((got - ref).abs() / ref.abs().max()).max()))
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": [row]}, f, indent=1)


if __name__ == "__main__":
    main()
