"""TK golden vectors: the REFERENCE TK_class (capreolus/reranker/TK.py, imported from the reference tree through _refharness) on the
numpy-seeded embeddings, weights and ids of tests/tk_case.py.  Records per pair the score and the 11 + 11 features (the inputs of
s_log_fcc / s_len_fcc, taken with forward hooks), the state_dict names and shapes, and for tk_grad the gradients of a fixed loss in
training mode with dropout p = 0.  Build container only; data out, no code.

    python tests/golden/make_golden_tk.py [CASE ...]     (from the repository root; no names: every case of tk_case.CASES)

usemask: the reference tiles its mask head-major while nn.MultiheadAttention's rows are batch-major, so in a batch of documents with
different masks a head reads another document's mask.  Masked cases are therefore recorded one document per call (the semantics the
engine implements for every document); unmasked cases are recorded as one batch.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import tk_case  # noqa: E402


def model(TK, name):
    m = TK.TK_class(tk_case.extractor(name), tk_case.config(name))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in tk_case.weights(name).items()}, strict=False)
    return m


def run(m, q, d):
    feats = {}
    h1 = m.s_log_fcc.register_forward_hook(lambda mod, inp, out: feats.__setitem__("log", inp[0].detach().clone()))
    h2 = m.s_len_fcc.register_forward_hook(lambda mod, inp, out: feats.__setitem__("len", inp[0].detach().clone()))
    score = m(torch.from_numpy(d), torch.from_numpy(q), None).view(-1)
    h1.remove()
    h2.remove()
    return score, feats["log"], feats["len"]


def gen(name, TK):
    torch.manual_seed(0)
    m = model(TK, name)
    q, d = tk_case.inputs(name)
    cfg = tk_case.config(name)
    out = {"query": q, "posdoc": d, "state_keys": np.array(sorted(m.state_dict())),
           "state_shapes": np.array([list(m.state_dict()[k].shape) + [0] * (3 - m.state_dict()[k].dim()) for k in sorted(m.state_dict())]),
           "pe_head": m.position_encoder.pe[:16, 0].numpy().copy()}
    for k, v in cfg.items():
        out["cfg." + k] = np.array(v)
    if name == "tk_grad":
        m.train()
        m.position_encoder.dropout.p = 0.0
        if cfg["usemask"]:
            score = torch.cat([m(torch.from_numpy(d[i:i + 1]), torch.from_numpy(q[i:i + 1]), None).view(-1) for i in range(q.shape[0])])
        else:
            score = m(torch.from_numpy(d), torch.from_numpy(q), None).view(-1)
        coef = torch.linspace(-1.0, 1.5, score.numel())
        (score * coef).sum().backward()
        out["score"] = score.detach().numpy()
        out["loss_coef"] = coef.numpy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["grad." + k] = p.grad.numpy().copy()
    else:
        m.eval()
        with torch.no_grad():
            if cfg["usemask"]:
                parts = [run(m, q[i:i + 1], d[i:i + 1]) for i in range(q.shape[0])]
                score, flog, flen = (torch.cat([p[j] for p in parts]) for j in range(3))
            else:
                score, flog, flen = run(m, q, d)
        out["score"], out["s_log_k"], out["s_len_k"] = score.numpy(), flog.numpy(), flen.numpy()
        s = out["score"]
        print(f"{name}: scores {np.round(s, 4)}; spread {s.max() - s.min():.4g}")
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)


def main():
    from _refharness import load_reference

    load_reference()
    TK = importlib.import_module("capreolus.reranker.TK")
    names = sys.argv[1:] or list(tk_case.CASES)
    unknown = [n for n in names if n not in tk_case.CASES]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {list(tk_case.CASES)}")
    for name in names:
        gen(name, TK)


if __name__ == "__main__":
    main()
