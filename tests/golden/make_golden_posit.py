"""POSITDRMM golden vectors: the REFERENCE POSITDRMM_class (capreolus/reranker/POSITDRMM.py, imported from the reference tree through
_refharness) on the numpy-seeded embeddings, weights, ids, idf and searcher scores of tests/posit_case.py, on the CPU in eval mode, with
`batch` set to the case's pair count (the reference takes no other batch size).  The extras handed to the model are the reference
plugin's own get_exact_match_stats (recorded as `stats`; for a query of one term, whose bigram list the reference cannot stack, its
get_exact_match_count and 0) next to the searcher scores.  Records per pair the score of test_forward and, from forward hooks, the
[B, Q, 6] input of Q1 and (where small; the pairs of posit_case.context_pairs) the two outputs of encoding_layer, batch first; the state_dict names and shapes; for posit_grad
the scores of forward(query, idf, pos, neg, ...) and the gradients of a fixed linear loss over them.  Build container only; data out,
no code.

    python tests/golden/make_golden_posit.py [CASE ...]     (from the repository root; no names: every case of posit_case.CASES)
"""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import posit_case  # noqa: E402


def model(ref, name):
    c = posit_case.CASES[name]
    m = ref.POSITDRMM_class(posit_case.extractor(name), {"batch": c["B"], "maxqlen": c["Q"], "maxdoclen": c["L"]})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in posit_case.weights(name).items()}, strict=False)
    return m.eval()


def stats(ref, idf, q, d):
    """[B, 3] from the reference plugin's own loops"""
    plugin = ref.POSITDRMM.__new__(ref.POSITDRMM)
    plugin.extractor = SimpleNamespace(pad=0)
    idf, q, d = torch.from_numpy(idf), torch.from_numpy(q), torch.from_numpy(d)
    if q.shape[1] > 1:
        return torch.cat(plugin.get_exact_match_stats(idf, q, d), dim=1).numpy()
    out = torch.zeros(d.shape[0], 3)
    for b in range(d.shape[0]):
        n, w = plugin.get_exact_match_count(q[b], plugin.clean(d[b]), idf[b])
        out[b, 0], out[b, 1] = n, w
    return out.numpy()


def gen(name, ref):
    torch.manual_seed(0)
    m = model(ref, name)
    ins = posit_case.inputs(name)
    q, d, idf, bm25 = ins[:4]
    posit_case.check_ids(q, d)
    st = stats(ref, idf, q, d)
    extras = np.concatenate([st, bm25[:, None]], axis=1).astype(np.float32)
    sd = m.state_dict()
    out = {"query": q, "posdoc": d, "query_idf": idf, "bm25": bm25, "stats": st, "extras": extras, "state_keys": np.array(sorted(sd)),
           "state_shapes": np.array([list(sd[k].shape) + [0] * (3 - sd[k].dim()) for k in sorted(sd)])}
    tq, td, tidf = torch.from_numpy(q), torch.from_numpy(d), torch.from_numpy(idf)
    if name == "posit_grad":
        neg, neg_bm25 = ins[4], ins[5]
        nst = stats(ref, idf, q, neg)
        nextras = np.concatenate([nst, neg_bm25[:, None]], axis=1).astype(np.float32)
        pos_s, neg_s = m(tq, tidf, td, torch.from_numpy(neg), torch.from_numpy(extras), torch.from_numpy(nextras))
        score = torch.cat([pos_s, neg_s])
        coef = torch.linspace(-1.0, 1.5, score.numel())
        (score * coef).sum().backward()
        out.update(negdoc=neg, neg_bm25=neg_bm25, neg_stats=nst, neg_extras=nextras, score=score.detach().numpy(), loss_coef=coef.numpy())
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["grad." + k] = p.grad.numpy().copy()
    else:
        seen = {"lstm": []}
        hooks = [m.posit1.Q1.register_forward_hook(lambda mod, inp, res: seen.__setitem__("features", inp[0].detach().clone())),
                 m.posit1.encoding_layer.register_forward_hook(lambda mod, inp, res: seen["lstm"].append(res[0].detach().clone()))]
        with torch.no_grad():
            score = m.test_forward(tq, tidf, td, torch.from_numpy(extras))
        for h in hooks:
            h.remove()
        out["score"], out["features"] = score.numpy(), seen["features"].numpy()
        if name in posit_case.CONTEXT_CASES:        # the query runs through the LSTM first, then the document; [S, B, 2 D] each
            out["lstm_query"], out["lstm_doc"] = (t.transpose(0, 1)[posit_case.context_pairs(name)].contiguous().numpy() for t in seen["lstm"])
        s = out["score"]
        print(f"{name}: scores {np.round(s, 4)}; spread {s.max() - s.min():.4g}")
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)


def main():
    from _refharness import load_reference

    load_reference()
    ref = importlib.import_module("capreolus.reranker.POSITDRMM")
    names = sys.argv[1:] or list(posit_case.CASES)
    unknown = [n for n in names if n not in posit_case.CASES]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {list(posit_case.CASES)}")
    for name in names:
        gen(name, ref)


if __name__ == "__main__":
    main()
