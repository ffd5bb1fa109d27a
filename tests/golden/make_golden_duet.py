"""DUET golden vectors: the REFERENCE DUET_class (capreolus/reranker/DUET.py, imported from the reference tree through _refharness) in
eval mode on the numpy-seeded embeddings, weights, ids and idf of tests/duet_case.py.  Records per pair the score, the two models' scores
(forward hooks on `lm` and `dm`), the query vector (`dm.q_ffw`) and the pooled map (`dm.d_conv1`, behind its MaxPool2d), the state_dict
names and shapes, and for duet_grad the scores of both documents and the gradients of a fixed linear loss over them.
`duet_sweep` records the same outputs at every point of duet_case.SWEEP (three pairs each) and at duet_case.LIMITS (two pairs), so that
the device tests know the reference's own fp32 error at each point.  Build container only; data out, no code.

    python tests/golden/make_golden_duet.py [CASE ...]     (from the repository root; no names: every case of duet_case.CASES and
                                                            duet_sweep)
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

from tests import duet_case  # noqa: E402


def model(DUET, cfg, ex, w):
    m = DUET.DUET_class(ex, dict(cfg, extractor=ex.config))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False)
    return m


def run(m, q, d, idf):
    """{score, lm, dm, qvec, pooled} of the reference model (numpy)"""
    seen = {}
    hooks = [mod.register_forward_hook(lambda _m, _i, res, k=k: seen.__setitem__(k, res.detach().clone()))
             for k, mod in (("lm", m.lm), ("dm", m.dm), ("qvec", m.dm.q_ffw), ("pooled", m.dm.d_conv1))]
    score = m(torch.from_numpy(d), torch.from_numpy(q), torch.from_numpy(idf)).view(-1)
    for h in hooks:
        h.remove()
    B = q.shape[0]
    return {"score": score.numpy(), "lm": seen["lm"].view(B).numpy(), "dm": seen["dm"].view(B).numpy(), "qvec": seen["qvec"].numpy(),
            "pooled": seen["pooled"][:, :, :, 0].numpy()}


def gen(name, DUET):
    torch.manual_seed(0)
    cfg = duet_case.config(name)
    m = model(DUET, cfg, duet_case.extractor(name), duet_case.weights(name))
    ids = duet_case.inputs(name)
    duet_case.check_ids(*ids[:3])
    sd = m.state_dict()
    out = {"query": ids[0], "posdoc": ids[1], "query_idf": ids[2], "state_keys": np.array(sorted(sd)),
           "state_shapes": np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in sorted(sd)])}
    for k, v in cfg.items():
        out["cfg." + k] = np.array(v)
    if name == "duet_grad":
        q, d, idf, neg = (torch.from_numpy(x) for x in ids)
        score = torch.cat([m(d, q, idf).view(-1), m(neg, q, idf).view(-1)])
        coef = torch.linspace(-1.0, 1.5, score.numel())
        (score * coef).sum().backward()
        out["negdoc"], out["score"], out["loss_coef"] = ids[3], score.detach().numpy(), coef.numpy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["grad." + k] = p.grad.numpy().copy()
    else:
        m.eval()
        with torch.no_grad():
            out.update(run(m, *ids))
        s = out["score"]
        print(f"{name}: scores {np.round(s, 4)}; lm {np.round(out['lm'], 3)}; dm {np.round(out['dm'], 3)}")
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)


def gen_sweep(DUET):
    out = {}
    for point in duet_case.SWEEP + (duet_case.LIMITS,):
        cfg, ex, w, q, d, idf = duet_case.sweep_case(*point, B=2 if point == duet_case.LIMITS else 3)
        m = model(DUET, cfg, ex, w).eval()
        with torch.no_grad():
            res = run(m, q, d, idf)
        key = duet_case.sweep_key(*point)
        for k, v in res.items():
            out[f"{k}.{key}"] = v
        print(f"duet_sweep {key}: scores {np.round(res['score'], 4)}")
    np.savez_compressed(os.path.join(HERE, "duet_sweep.npz"), **out)


def main():
    from _refharness import load_reference

    load_reference()
    DUET = importlib.import_module("capreolus.reranker.DUET")
    known = list(duet_case.CASES) + ["duet_sweep"]
    names = sys.argv[1:] or known
    unknown = [n for n in names if n not in known]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {known}")
    for name in names:
        if name == "duet_sweep":
            gen_sweep(DUET)
        else:
            gen(name, DUET)


if __name__ == "__main__":
    main()
