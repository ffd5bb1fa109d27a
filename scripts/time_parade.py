"""PARADE throughput at the reproduction's shape (BERT-base, 16 passages x 256 tokens per document): documents/s and passages/s of
PTParade.test, MaxP's passages/s on the same inputs in the same run (alternating calls), and the aggregation head's own time
(capamd_parade_head alone on the call's [CLS] rows).  HIP events after warm-up.

    python scripts/time_parade.py [--batches 16,64] [--dtypes fp16,bf16] [--iters 10] [--out profiles/parade/time_parade.json]
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

from capreolus_amd import synthetic  # noqa: E402
from capreolus_amd.reranker import PTBERTMaxP, PTParade  # noqa: E402
from tests.parade_case import parade_head_weights  # noqa: E402

DIMS = dict(hidden=768, layers=12, heads=12, ffn=3072, vocab=30522, max_pos=512)


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
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P, S, dev = 16, 256, "cuda:0"
    w = synthetic.random_bert_weights(seed=7, **DIMS)
    head = {k: v.to(dev) for k, v in parade_head_weights(7, 768, 3072, P, w["bert.embeddings.word_embeddings.weight"]).items()}
    rows = []
    for dt in a.dtypes.split(","):
        ext = SimpleNamespace(config={"numpassages": P, "maxseqlen": S})
        par = PTParade({"pretrained": dict(DIMS), "compute_dtype": dt}, ext)
        pm = par.build_model()
        pm.bert.load_state_dict({k[5:]: v for k, v in w.items() if k.startswith("bert.")}, strict=False)
        pm.load_state_dict({k: v.cpu() for k, v in head.items()}, strict=False)
        pm.to(dev).eval()
        mx = PTBERTMaxP({"pretrained": dict(DIMS), "compute_dtype": dt}, ext)
        mm = mx.build_model()
        mm.bert.load_state_dict(w, strict=False)
        mm.to(dev).eval()
        for B in (int(x) for x in a.batches.split(",")):
            psg = synthetic.make_bert_passages(np.random.RandomState(B), B, P, S, vocab=DIMS["vocab"])
            d = {k: torch.as_tensor(v).to(dev) for k, v in psg.items()}
            with torch.no_grad():
                eng = pm.engine()
                for _ in range(a.warmup):
                    par.test(d), mx.test(d)
                t_par, t_max = [], []
                for _ in range(3):           # alternating, so that clocks and caches treat both alike
                    t_par.append(timed(lambda: par.test(d), a.iters))
                    t_max.append(timed(lambda: mx.test(d), a.iters))
                _, cls = eng.forward(d["pos_bert_input"], d["pos_mask"], d["pos_seg"], pm.head_params(), return_cls=True)
                hp = pm.head_params()
                t_head = timed(lambda: eng.head(cls, B, P, hp), a.iters * 5)
            tp, tm = float(np.median(t_par)), float(np.median(t_max))
            row = dict(dtype=dt, B=B, P=P, S=S, parade_s=tp, parade_docs_per_s=B / tp, parade_passages_per_s=B * P / tp, maxp_s=tm,
                       maxp_passages_per_s=B * P / tm, parade_over_maxp=tm / tp, head_s=t_head, head_share=t_head / tp)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
