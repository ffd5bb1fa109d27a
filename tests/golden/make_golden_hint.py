"""HINT golden vectors: the REFERENCE HiNT_main (capreolus/reranker/HINT.py, imported from the reference tree through _refharness) on
the numpy-seeded embeddings, weights and ids of tests/hint_case.py, with `batch` set to the case's pair count (the reference takes no
other batch size).  Records per pair the score of test_forward and the [P, B, 8] input of HiNT1.lstm (a forward hook), the state_dict
names and shapes, and for hint_grad the scores of forward(query, idf, pos, neg) and the gradients of a fixed loss over them.
`hint_sweep` records the reference's scores and LSTM input at every (Q, L) of hint_case.SWEEP (three pairs each; the ids and weights
are hint_case.sweep_case's), so that the device tests know the reference's own fp32 error at each point.  Build container only; data
out, no code.

    python tests/golden/make_golden_hint.py [CASE ...]     (from the repository root; no names: every case of hint_case.CASES and
                                                            hint_sweep)
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

from tests import hint_case  # noqa: E402


def model(HINT, name):
    c = hint_case.CASES[name]
    cfg = dict(hint_case.config(name), maxqlen=c["Q"], maxdoclen=c["L"], batch=c["B"])
    m = HINT.HiNT_main(hint_case.extractor(name), cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in hint_case.weights(name).items()}, strict=False)
    return m


def gen(name, HINT):
    torch.manual_seed(0)
    m = model(HINT, name)
    ids = hint_case.inputs(name)
    hint_case.check_ids(ids[0], ids[1])
    q, d = torch.from_numpy(ids[0]), torch.from_numpy(ids[1])
    idf = torch.zeros(q.shape)
    sd = m.state_dict()
    out = {"query": ids[0], "posdoc": ids[1], "state_keys": np.array(sorted(sd)),
           "state_shapes": np.array([list(sd[k].shape) + [0] * (3 - sd[k].dim()) for k in sorted(sd)])}
    for k, v in hint_case.config(name).items():
        out["cfg." + k] = np.array(v)
    if name == "hint_grad":
        neg = torch.from_numpy(ids[2])
        pos_s, neg_s = m(q, idf, d, neg)
        score = torch.cat([pos_s, neg_s])
        coef = torch.linspace(-1.0, 1.5, score.numel())
        (score * coef).sum().backward()
        out["negdoc"], out["score"], out["loss_coef"] = ids[2], score.detach().numpy(), coef.numpy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["grad." + k] = p.grad.numpy().copy()
    else:
        seen = {}
        h = m.HiNT1.lstm.register_forward_hook(lambda mod, inp, res: seen.__setitem__("ev", inp[0].detach().clone()))
        with torch.no_grad():
            score = m.test_forward(q, idf, d)
        h.remove()
        out["score"], out["evidence"] = score.numpy(), seen["ev"].numpy()
        s = out["score"]
        print(f"{name}: scores {np.round(s, 4)}; spread {s.max() - s.min():.4g}")
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)


def gen_sweep(HINT):
    out = {}
    for Q, L in hint_case.SWEEP:
        cfg, ex, w, q, d = hint_case.sweep_case(Q, L)
        m = HINT.HiNT_main(ex, dict(cfg, maxqlen=Q, maxdoclen=L, batch=q.shape[0]))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
        seen = {}
        h = m.HiNT1.lstm.register_forward_hook(lambda mod, inp, res: seen.__setitem__("ev", inp[0].detach().clone()))
        with torch.no_grad():
            score = m.test_forward(torch.from_numpy(q), torch.zeros(q.shape), torch.from_numpy(d))
        h.remove()
        out[f"score.{Q}.{L}"], out[f"evidence.{Q}.{L}"] = score.numpy(), seen["ev"].numpy()
        print(f"hint_sweep Q {Q} L {L}: scores {np.round(score.numpy(), 4)}")
    np.savez_compressed(os.path.join(HERE, "hint_sweep.npz"), **out)


def main():
    from _refharness import load_reference

    load_reference()
    HINT = importlib.import_module("capreolus.reranker.HINT")
    names = sys.argv[1:] or list(hint_case.CASES) + ["hint_sweep"]
    unknown = [n for n in names if n not in hint_case.CASES and n != "hint_sweep"]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {list(hint_case.CASES) + ['hint_sweep']}")
    for name in names:
        if name == "hint_sweep":
            gen_sweep(HINT)
        else:
            gen(name, HINT)


if __name__ == "__main__":
    main()
