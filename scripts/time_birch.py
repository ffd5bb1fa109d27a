"""Birch throughput at BERT-large (24 layers, 1024 hidden, 16 heads, 4096 FFN), 16 passages x 256 tokens per document, 1000 candidates
scored in calls of --batch documents, in both `truncate` modes: passages/s over the ENCODED passages, the share of passage slots that
are never encoded, the time of capamd_birch_plan and capamd_birch_head alone, and an eager restatement of the reference's forward
(birch.py:72-127: per document, sub-batches of `batch` passages through transformers' BertForNextSentencePrediction under fp16 autocast;
for truncate = "none" the same without the cut) on the same GPU over the first --eager-docs candidates.  HIP events after warm-up.

    python scripts/time_birch.py [--candidates 1000] [--batch 100] [--iters 2] [--eager-docs 100] [--out profiles/birch/time_birch.json]
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
from capreolus_amd.reranker import Birch  # noqa: E402

DIMS = dict(hidden=1024, layers=24, heads=16, ffn=4096, vocab=30522, max_pos=512)


def timed(fn, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_time(ev[1]) / iters / 1e3


def eager_forward(hf, combine_w, doc, seg, mask, topk, truncate):
    """the reference's forward in plain PyTorch (its own loop structure), fp16 autocast"""
    batch = doc.shape[0]
    scores = []
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for b in range(batch):
            valid = ((seg[b] + mask[b]) == 2).sum(dim=1) > 2
            if not valid.any():
                valid[0] = True
            d, s, m = doc[b][valid], seg[b][valid], mask[b][valid]
            out = []
            for i in range(0, d.shape[0], batch):
                sd, ss, sm = d[i:i + batch], s[i:i + batch], m[i:i + batch]
                if truncate == "reference":
                    idx = (ss + sm).argmax(dim=1).max()
                    sd, ss, sm = sd[:, :idx + 1], ss[:, :idx + 1], sm[:, :idx + 1]
                out.append(hf(input_ids=sd, token_type_ids=ss, attention_mask=sm)[0][:, 1].float())
            real = torch.cat(out)
            scores.append(torch.cat([real, real.min().repeat(doc.shape[1] - real.shape[0])]))
        top = torch.topk(torch.stack(scores), k=topk, dim=1).values
        return top @ combine_w.view(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--eager-docs", type=int, default=100)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--layers", type=int, default=DIMS["layers"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    P, S, dev, N = 16, 256, "cuda:0", a.candidates
    dims = dict(DIMS, layers=a.layers)
    w = synthetic.random_bert_weights(seed=7, **dims)
    bert = {k: v for k, v in w.items() if k.startswith("bert.")}
    bert["cls.seq_relationship.weight"], bert["cls.seq_relationship.bias"] = w["classifier.weight"], w["classifier.bias"]
    psg = synthetic.make_bert_passages(np.random.RandomState(1), N, P, S, vocab=dims["vocab"], same_query=False)
    d = {k: torch.as_tensor(v).to(dev) for k, v in psg.items()}
    calls = [{k: v[i:i + a.batch] for k, v in d.items()} for i in range(0, N, a.batch)]
    try:
        from transformers import BertConfig, BertForNextSentencePrediction

        hf = BertForNextSentencePrediction(BertConfig(hidden_size=dims["hidden"], num_hidden_layers=dims["layers"], num_attention_heads=dims["heads"],
                                                      intermediate_size=dims["ffn"], vocab_size=dims["vocab"], max_position_embeddings=dims["max_pos"]))
        hf.load_state_dict(bert, strict=False)
        hf.to(dev).eval()
    except ImportError:
        hf = None
    rows = []
    ext = SimpleNamespace(config={"numpassages": P, "maxseqlen": S})
    for truncate in ("reference", "none"):
        r = Birch({"pretrained": dict(dims), "compute_dtype": a.dtype, "truncate": truncate}, ext)
        m = r.build_model()
        m.bert.load_state_dict(bert, strict=False)
        m.to(dev).eval()
        eng = m.engine()
        topk = r.config["topk"]
        with torch.no_grad():
            run = lambda: [r.test(c) for c in calls]
            for _ in range(a.warmup):
                run()
            t = timed(run, a.iters)
            c0 = calls[0]
            B0 = c0["pos_bert_input"].shape[0]
            plan = lambda: eng.plan(c0["pos_bert_input"], c0["pos_mask"], c0["pos_seg"], B0)
            n_enc = sum(int(eng.plan(c["pos_bert_input"], c["pos_mask"], c["pos_seg"], c["pos_bert_input"].shape[0])[3][-1]) for c in calls)
            t_plan = timed(plan, 20)
            e_ids, e_mask, e_seg, doc_first = plan()
            logits = eng.passage_logits(e_ids, e_mask, e_seg)
            cp = m.combine_params()
            t_head = timed(lambda: eng.head(logits, doc_first, B0, P, topk, cp), 50)
            row = dict(truncate=truncate, dtype=a.dtype, layers=dims["layers"], candidates=N, batch=a.batch, P=P, S=S, seconds=t, docs_per_s=N / t,
                       encoded_passages=n_enc, passages_per_s=n_enc / t, slots_skipped_share=1.0 - n_enc / (N * P),
                       plan_s_per_call=t_plan, head_s_per_call=t_head, plan_and_head_share=(t_plan + t_head) * len(calls) / t)
            if hf is not None and a.eager_docs > 0:
                ne = min(a.eager_docs, N) // a.batch * a.batch or min(a.eager_docs, N)
                ecalls = [{k: v[i:i + a.batch] for k, v in d.items()} for i in range(0, ne, a.batch)]
                eager = lambda: [eager_forward(hf, m.combine.weight, c["pos_bert_input"], c["pos_seg"], c["pos_mask"], topk, truncate) for c in ecalls]
                eager()
                te = timed(eager, 1)
                enc_e = sum(int(eng.plan(c["pos_bert_input"], c["pos_mask"], c["pos_seg"], c["pos_bert_input"].shape[0])[3][-1]) for c in ecalls)
                got = torch.cat([r.test(c) for c in ecalls])
                row.update(eager_docs=ne, eager_seconds=te, eager_passages_per_s=enc_e / te, engine_over_eager=(n_enc / t) / (enc_e / te),
                           max_abs_diff_to_eager=float((got - torch.cat(eager())).abs().max()))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del r, m, eng
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
