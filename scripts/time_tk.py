"""TK throughput at the reproduction's shape (4 query x 800 document terms, 300-d embeddings, 1000 candidates per call), defaults and
usemask=True: documents/s of TK.test (capamd_tk_forward), executed (padded) and nominal GFLOP per document, the fraction of the
157.3 TF fp32 matrix peak, and the eager PyTorch restatement (TK_class._forward_aten, fp32, on the same GPU, in chunks of documents
so that its [chunk, heads, L, L] score tensors fit) on the same inputs as the speedup's denominator.  HIP events after warm-up.

    python scripts/time_tk.py [--candidates 1000] [--iters 5] [--no-eager] [--out profiles/tk/time_tk.json]

Kernel shares: run it under `rocprofv3 --kernel-trace --stats -- python scripts/time_tk.py --no-eager --iters 3` (profiles/tk/).
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

from capreolus_amd.reranker import TK  # noqa: E402

PEAK_FP32 = 157.3e12


def timed(fn, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / iters / 1e3


def flops_per_doc(D, heads, F, layers, Q, L, padded):
    """multiply-adds x 2 of the encoder over one document and one query (both sides) plus the cosine matrix"""
    hd = D // heads
    if padded:
        up = lambda n: (n + 63) // 64 * 64
        Dw, hs, Fw = up(D), (hd + 15) // 16 * 16, up(F)
        Hs = up(heads * hs)
    else:
        Dw, hs, Fw, Hs = D, hd, F, D
    def side(S):
        gemm = 2 * S * (3 * Hs * Dw + Dw * Hs + 2 * Fw * Dw)
        attn = 4 * S * S * heads * hs
        return layers * (gemm + attn)
    return side(L) + side(Q) + 2 * Q * L * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--eager-chunk", type=int, default=25)
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
    rows = []
    for usemask in (False, True):
        r = TK({"usemask": usemask}, SimpleNamespace(embeddings=emb, pad=0))
        m = r.build_model().to(dev).eval()
        with torch.no_grad():
            for _ in range(a.warmup):
                r.test(batch)
            t = float(np.median([timed(lambda: r.test(batch), a.iters) for _ in range(3)]))
            t_eager = None
            if not a.no_eager:
                def eager():
                    for i in range(0, B, a.eager_chunk):
                        m._forward_aten(d[i:i + a.eager_chunk], q[i:i + a.eager_chunk])
                eager()
                t_eager = timed(eager, 1)
                got = r.test(batch)
                ref = torch.cat([m._forward_aten(d[i:i + a.eager_chunk], q[i:i + a.eager_chunk]) for i in range(0, B, a.eager_chunk)])
                max_rel = float(((got - ref).abs() / ref.abs().max()).max())
        ex, nom = flops_per_doc(D, 10, 100, 2, Q, L, True), flops_per_doc(D, 10, 100, 2, Q, L, False)
        row = dict(usemask=usemask, candidates=B, Q=Q, L=L, D=D, call_s=t, docs_per_s=B / t, executed_gflop_per_doc=ex / 1e9,
                   nominal_gflop_per_doc=nom / 1e9, executed_tflops=ex * B / t / 1e12, fraction_of_fp32_peak=ex * B / t / PEAK_FP32,
                   nominal_fraction_of_fp32_peak=nom * B / t / PEAK_FP32)
        if t_eager is not None:
            row.update(eager_s=t_eager, eager_docs_per_s=B / t_eager, speedup_over_eager=t_eager / t, max_rel_diff_vs_eager=max_rel)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
