"""HINT throughput at the reproduction's shape (4 query x 800 document terms, 300-d embeddings, 1000 candidates per call, documents of
mixed real length): documents/s of HINT.test (capamd_hint_forward), spatial-GRU cell updates/s, and the eager PyTorch restatement
(HiNT_main._forward_aten, fp32, on the same GPU, on the same inputs, in chunks of documents) as the speedup's denominator.  HIP events
after warm-up, median of three; the eager run is launch-bound (one round of ATen calls per cell whatever the batch) and runs once.

    python scripts/time_hint.py [--candidates 1000] [--iters 5] [--no-eager] [--out profiles/hint/time_hint.json]

Stage shares: run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_hint.py --no-eager --iters 3` (profiles/hint/).
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

from capreolus_amd.reranker import HINT  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
    batch = {"query": q, "posdoc": d, "query_idf": torch.zeros((B, Q), device=dev)}
    torch.manual_seed(0)
    r = HINT({}, SimpleNamespace(embeddings=emb, pad=0, config={"maxqlen": Q, "maxdoclen": L}))
    m = r.build_model().to(dev).eval()
    P = L // 100
    cells = B * P * 4 * Q * 100             # windows x {xor, cos} x {forward, reversed} chains of Q x 100 cells
    with torch.no_grad():
        for _ in range(a.warmup):
            r.test(batch)
        t = float(np.median([timed(lambda: r.test(batch), a.iters) for _ in range(3)]))
        row = dict(candidates=B, Q=Q, L=L, D=D, windows=P, call_s=t, docs_per_s=B / t, gru_cells_per_call=cells, gru_cells_per_s=cells / t)
        if not a.no_eager:
            def eager():
                return torch.cat([m._forward_aten(d[i:i + a.eager_chunk], q[i:i + a.eager_chunk]) for i in range(0, B, a.eager_chunk)])
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            ref = eager()
            ev[1].record()
            ev[1].synchronize()
            t_eager = ev[0].elapsed_time(ev[1]) / 1e3
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
