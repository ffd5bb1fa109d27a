"""CDSSM golden vectors: the REFERENCE CDSSM_class (capreolus/reranker/CDSSM.py, imported from the reference tree through _refharness)
on the numpy-seeded embeddings, weights and ids of tests/cdssm_case.py.  Records per pair the score and the two tower outputs (the
max over everything a forward hook on `conv` saw for a side: the reference calls it once per window, the query's windows first), the
state_dict names and shapes, and for cdssm_grad the scores of both documents and the gradients of a fixed loss over them.
`cdssm_sweep` records the reference's scores and tower outputs at every point of cdssm_case.SWEEP (three pairs each), so that the device
tests know the reference's own fp32 error at each point.  Build container only; data out, no code.

    python tests/golden/make_golden_cdssm.py [CASE ...]     (from the repository root; no names: every case of cdssm_case.CASES and
                                                             cdssm_sweep)
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

from tests import cdssm_case  # noqa: E402


def run(m, q, d):
    """(scores [B], query tower [B, R], document tower [B, R]) of the reference model"""
    seen = []
    h = m.conv.register_forward_hook(lambda mod, inp, res: seen.append(res.detach().clone()))
    score = m(torch.from_numpy(d), torch.from_numpy(q)).view(-1)
    h.remove()
    W = m.p["windowsize"]
    kq = q.shape[1] // W + 1
    assert len(seen) == kq + d.shape[1] // W + 1, len(seen)
    towers = [torch.cat(part, dim=1).max(dim=1)[0].numpy() for part in (seen[:kq], seen[kq:])]
    return score, towers[0], towers[1]


def model(CDSSM, cfg, ex, w):
    m = CDSSM.CDSSM_class(ex, cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    return m


def gen(name, CDSSM):
    torch.manual_seed(0)
    m = model(CDSSM, cdssm_case.config(name), cdssm_case.extractor(name), cdssm_case.weights(name))
    ids = cdssm_case.inputs(name)
    cdssm_case.check_ids(ids[0], ids[1])
    sd = m.state_dict()
    out = {"query": ids[0], "posdoc": ids[1], "state_keys": np.array(sorted(sd)),
           "state_shapes": np.array([list(sd[k].shape) + [0] * (3 - sd[k].dim()) for k in sorted(sd)])}
    for k, v in cdssm_case.config(name).items():
        out["cfg." + k] = np.array(v)
    if name == "cdssm_grad":
        q, d, neg = (torch.from_numpy(x) for x in ids)
        score = torch.cat([m(d, q).view(-1), m(neg, q).view(-1)])
        coef = torch.linspace(-1.0, 1.5, score.numel())
        (score * coef).sum().backward()
        out["negdoc"], out["score"], out["loss_coef"] = ids[2], score.detach().numpy(), coef.numpy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["grad." + k] = p.grad.numpy().copy()
    else:
        with torch.no_grad():
            score, qt, dt = run(m, ids[0], ids[1])
        out["score"], out["qtower"], out["dtower"] = score.numpy(), qt, dt
        s = out["score"]
        print(f"{name}: scores {np.round(s, 4)}; spread {s.max() - s.min():.4g}")
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)


def gen_sweep(CDSSM):
    out = {}
    for point in cdssm_case.SWEEP:
        cfg, ex, w, q, d = cdssm_case.sweep_case(*point)
        m = model(CDSSM, cfg, ex, w)
        with torch.no_grad():
            score, qt, dt = run(m, q, d)
        key = cdssm_case.sweep_key(*point)
        out["score." + key], out["qtower." + key], out["dtower." + key] = score.numpy(), qt, dt
        print(f"cdssm_sweep {key}: scores {np.round(score.numpy(), 4)}")
    np.savez_compressed(os.path.join(HERE, "cdssm_sweep.npz"), **out)


def main():
    from _refharness import load_reference

    load_reference()
    CDSSM = importlib.import_module("capreolus.reranker.CDSSM")
    names = sys.argv[1:] or list(cdssm_case.CASES) + ["cdssm_sweep"]
    unknown = [n for n in names if n not in cdssm_case.CASES and n != "cdssm_sweep"]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {list(cdssm_case.CASES) + ['cdssm_sweep']}")
    for name in names:
        if name == "cdssm_sweep":
            gen_sweep(CDSSM)
        else:
            gen(name, CDSSM)


if __name__ == "__main__":
    main()
