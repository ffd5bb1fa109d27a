"""DUET throughput at the reproduction's shape, 1000 candidates of one query per call: 4 query x 800 document terms, 300-d embeddings over
a vocabulary of 400,001, the default configuration (nfilters 10, lmhidden 30, nhidden 699, relu, idfweight).  DUET.test (one
capamd_duet_forward call: proj_kernel + doc_kernel, csrc/duet.hip) is timed against the plugin's eager PyTorch restatement
(_forward_aten, fp32, same GPU, same inputs) in the same process, the two legs interleaved round by round so that a neighbour's load on
the machine falls on both: HIP events around `--iters` calls, the median of `--rounds` rounds.  Two draws of document ids, since the row
gather is what the projection kernel waits for beside its arithmetic:
  uniform  every term uniform over the vocabulary: almost every row of a call is distinct and comes from HBM;
  zipf     Zipf 1.1 over the vocabulary, as text is: most rows are re-read from cache.
Next to every time the compulsory work is printed - what the kernels cannot avoid - and the time it takes at this chip's rates:
  gathered bytes: every embedding row the ids name, read once (rows x dim x 4), and the time at the 6.3 TB/s its HBM reaches;
  hbm bytes: the ids, the DISTINCT rows, the projections written and read back once, the outputs;
  flops: 2 x 3 H dim per document term (the projections; everything else is under 2 % of it), and the time at the fp32 vector rate.
After the timed rounds, in a pass of its own, torch.profiler lists the device time of every kernel of `--iters` engine calls: the
per-kernel split (the profiler slows the host, so the end-to-end figures are taken without it).  Run it under ONE time limit
(`timeout -k 10 600 python scripts/time_duet.py ...`).

    python scripts/time_duet.py [--candidates 1000] [--iters 5] [--rounds 5] [--no-eager] [--no-split] [--out profiles/duet/time_duet.json]
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

from capreolus_amd.reranker import DUET  # noqa: E402

HBM_BYTES_PER_S = 6.3e12        # what a streaming copy reaches on this chip (8 TB/s on paper)
FP32_FLOPS_PER_S = 157.3e12     # the fp32 vector rate on paper (256 CUs x 128 lanes x 2 flops x 2.4 GHz, packed)


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


def kernel_split(fn, iters):
    """{kernel name: seconds per call} of the device kernels of `iters` calls, by torch.profiler"""
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        if t is None:
            t = getattr(e, "cuda_time_total", 0.0)
        if t > 0:
            split[e.key] = float(t) / 1e6 / iters
    if not split:
        raise RuntimeError("the profiler recorded no device kernel")
    return split


def draw(kind, rs, B, L, V):
    if kind == "uniform":
        d = rs.randint(1, V, size=(B, L))
    else:
        d = np.minimum(rs.zipf(1.1, size=(B, L)), V - 1)
    lens = rs.randint(L // 4, L + 1, size=B)
    for i in range(B):                      # documents of the extractor's shape: real terms, then pads
        d[i, int(lens[i]):] = 0
    return torch.from_numpy(d.astype(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--vocab", type=int, default=400001)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_duet.py measures on an MI355X; no GPU is visible (nothing is measured on the host)")
    dev = "cuda:0"
    V, D, Q, L, B = a.vocab, 300, 4, 800, a.candidates
    emb = np.random.default_rng(0).standard_normal((V, D), dtype=np.float32) * 0.5
    emb[0] = 0
    torch.manual_seed(0)
    r = DUET({}, SimpleNamespace(embeddings=emb, pad=0, config={"maxqlen": Q, "maxdoclen": L}))
    m = r.build_model().to(dev).eval()
    H = r.config["nfilters"]
    rs = np.random.RandomState(0)
    q = torch.from_numpy(rs.randint(1, V, size=(1, Q))).repeat(B, 1).to(dev)
    idf = torch.from_numpy(rs.uniform(0.5, 3.0, size=(1, Q)).astype(np.float32)).repeat(B, 1).to(dev)
    rows = []
    for kind in ("uniform", "zipf"):
        d = draw(kind, rs, B, L, V).to(dev)
        batch = {"query": q, "posdoc": d, "query_idf": idf}
        legs = {"test": lambda: r.test(batch)}
        if not a.no_eager:
            legs["eager"] = lambda: m._forward_aten(d, q, idf)
        with torch.no_grad():
            t, spread = interleaved(legs, a.iters, a.rounds, a.warmup)
            got = r.test(batch)
            diff = None if a.no_eager else float((got - m._forward_aten(d, q, idf)).abs().max())
            scale = float(got.abs().max())
            split, split_error = None, None
            if not a.no_split:
                try:
                    split = kernel_split(lambda: r.test(batch), a.iters)
                except Exception as e:      # the split is an extra: the end-to-end figures above stand without it
                    split_error = f"{type(e).__name__}: {e}"
        gathered = (B * L + B * Q) * D * 4
        distinct = int(torch.unique(torch.cat([d.reshape(-1), q.reshape(-1)])).numel())
        OP = (3 * H + 15) // 16 * 16
        hbm = (B * L + B * Q) * 8 + distinct * D * 4 + 2 * B * L * OP * 4 + B * 4
        flops = 2 * B * L * 3 * H * D
        row = dict(model="DUET", ids=kind, candidates=B, Q=Q, L=L, D=D, vocab=V, nfilters=H, call_s=t["test"], docs_per_s=B / t["test"],
                   score_scale=scale, gathered_bytes=gathered, gathered_floor_s=gathered / HBM_BYTES_PER_S, distinct_rows=distinct, hbm_bytes=hbm,
                   hbm_floor_s=hbm / HBM_BYTES_PER_S, projection_flops=flops, flops_floor_s=flops / FP32_FLOPS_PER_S, rounds=spread,
                   kernel_split_s=split, kernel_split_error=split_error)
        if not a.no_eager:
            row.update(eager_s=t["eager"], speedup_over_eager=t["eager"] / t["test"], max_abs_diff_vs_eager=diff)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
