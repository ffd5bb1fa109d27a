"""DSSM golden vectors: the REFERENCE DSSM_class (capreolus/reranker/DSSM.py, imported from the reference tree through _refharness) on
the numpy-seeded weights and bags of tests/dssm_case.py, fed the dense [B, nvocab] matrices it reads.  Records the bags in SPARSE form
(indptr, idx, val per side - never the dense matrix), per pair the score and the two tower outputs (a forward hook on `ffw`: the
reference calls it for the query first), the state_dict names and shapes, and for dssm_grad the scores of both documents and the
gradients of a fixed loss over them - with the model in eval mode, so that the reference's Dropout(0.5) is the identity and the
gradients are those of the function itself.  Build container only; data out, no code.

    python tests/golden/make_golden_dssm.py [CASE ...]     (from the repository root; no names: every case of dssm_case.CASES)
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

from tests import dssm_case  # noqa: E402


def gen(name, DSSM):
    torch.manual_seed(0)
    nvocab = dssm_case.CASES[name]["nvocab"]
    m = DSSM.DSSM_class(dssm_case.extractor(name), dssm_case.config(name))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in dssm_case.weights(name).items()})
    m.eval()
    bags = dssm_case.inputs(name)
    dssm_case.check_bags(bags[0], bags[1], nvocab)
    sd = m.state_dict()
    out = {"nvocab": np.array(nvocab), "state_keys": np.array(sorted(sd)),
           "state_shapes": np.array([list(sd[k].shape) + [0] * (2 - sd[k].dim()) for k in sorted(sd)])}
    for side, bag in zip(("query", "posdoc", "negdoc"), bags):
        out[side + ".indptr"], out[side + ".idx"], out[side + ".val"] = bag
    for k, v in dssm_case.config(name).items():
        out["cfg." + k] = np.array(v)
    q, d = (torch.from_numpy(dssm_case.dense(b, nvocab)) for b in bags[:2])
    idf = torch.zeros(q.shape[0], 4)
    if name == "dssm_grad":
        neg = torch.from_numpy(dssm_case.dense(bags[2], nvocab))
        score = torch.cat([m(d, q, idf).view(-1), m(neg, q, idf).view(-1)])
        coef = torch.linspace(-1.0, 1.5, score.numel())
        (score * coef).sum().backward()
        out["score"], out["loss_coef"] = score.detach().numpy(), coef.numpy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["grad." + k] = p.grad.numpy().copy()
    else:
        seen = []
        h = m.ffw.register_forward_hook(lambda mod, inp, res: seen.append(res.detach().clone().numpy()))
        with torch.no_grad():
            score = m(d, q, idf).view(-1)
        h.remove()
        out["score"], out["qtower"], out["dtower"] = score.numpy(), seen[0], seen[1]
        s = out["score"]
        print(f"{name}: scores {np.round(s, 4)}; spread {s.max() - s.min():.4g}")
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)


def main():
    from _refharness import load_reference

    load_reference()
    DSSM = importlib.import_module("capreolus.reranker.DSSM")
    names = sys.argv[1:] or list(dssm_case.CASES)
    unknown = [n for n in names if n not in dssm_case.CASES]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {list(dssm_case.CASES)}")
    for name in names:
        gen(name, DSSM)


if __name__ == "__main__":
    main()
