"""DeepTileBar golden vectors: the REFERENCE DeepTileExtractor.create_visualization_matrix (capreolus/extractor/deeptileextractor.py)
and DeepTileBar_class (capreolus/reranker/DeepTileBar.py), imported from the reference tree through _refharness, on the numpy-seeded
vocabulary, embeddings, idf, weights, query tokens and segment strings of tests/deeptile_case.py, with `batch` set to the case's
document count (the reference takes no other batch size).  The extractor is made with object.__new__ and its attributes set by hand:
nothing of its indexing, tokenising or tiling runs.  Records per case the strings, their ids and offsets, the reference's tiles, the
scores of test_forward, the input of W1 (a forward pre-hook), the state_dict names and shapes, and for deeptile_grad the scores of
forward(pos, neg) and the gradients of a fixed loss over them.  Build container only; data out, no code.

    python tests/golden/make_golden_deeptile.py [CASE ...]     (from the repository root; no names: every case of deeptile_case.CASES)
"""
import importlib
import os
import pathlib
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import deeptile_case  # noqa: E402


def load_reference_deeptile():
    """(extractor module, reranker module) of the reference, with stand-ins for the third-party modules the build container lacks and for the
    capreolus.extractor package base (its real __init__ pulls in the whole module graph)"""
    import _refharness
    from _refharness import REF_ROOT, _stub, load_reference

    load_reference()
    cap = sys.modules["capreolus"]
    cap.constants = {"CACHE_BASE_PATH": pathlib.Path("/nonexistent")}

    class _Never:
        def __init__(self, *a, **k):
            raise RuntimeError("a stand-in: the real module is not installed")

    _stub("nltk", TextTilingTokenizer=_Never)
    _stub("pymagnitude", Magnitude=_Never, MagnitudeUtils=_Never)
    for name in ("spacy", "requests", "profane"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                _stub(name)

    class Extractor(cap.ModuleBase):
        pass

    ex = _stub("capreolus.extractor", Extractor=Extractor)
    ex.__path__ = [os.path.join(REF_ROOT, "capreolus", "extractor")]
    cap.extractor = ex
    assert _refharness.REF_ROOT == REF_ROOT
    return importlib.import_module("capreolus.extractor.deeptileextractor"), importlib.import_module("capreolus.reranker.DeepTileBar")


def reference_extractor(DTE, name):
    ref = deeptile_case.extractor(name)
    ex = object.__new__(DTE.DeepTileExtractor)
    ex.config = dict(ref.config)      # (tilechannels set to the case's C: with tfchannel false and the default 3 it cannot build the tile)
    ex.stoi, ex.idf, ex.embeddings = ref.stoi, ref.idf, ref.embeddings
    return ex


def reference_tiles(ex, queries, docs):
    return torch.stack([ex.create_visualization_matrix(q, segs, ex.embeddings) for q, segs in zip(queries, docs)])     # [B, 1, Q, P, C]


def gen(name, DTE, DTB):
    torch.manual_seed(0)
    c = deeptile_case.CASES[name]
    deeptile_case.check_text(name)
    ex = reference_extractor(DTE, name)
    m = DTB.DeepTileBar_class(ex, dict(deeptile_case.config(name), batch=c["B"]))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in deeptile_case.weights(name).items()}, strict=True)
    queries, docs = deeptile_case.text(name)
    q, idf, d, off = deeptile_case.encode(name)
    tiles = reference_tiles(ex, queries, docs)
    sd = m.state_dict()
    out = {"query": q, "query_idf": idf, "posdoc": d, "posdoc_segments": off, "query_toks": np.array(queries), "segments": np.array(docs),
           "tiles": tiles[:, 0].numpy(), "state_keys": np.array(sorted(sd)),
           "state_shapes": np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in sorted(sd)])}
    for k, v in list(deeptile_case.config(name).items()) + list(deeptile_case.extractor_config(name).items()):
        out["cfg." + k] = np.array(v)
    batch = {"qid": list(range(c["B"])), "posdoc": tiles}
    if name == "deeptile_grad":
        nq, ndocs = deeptile_case.text(name, negative=True)
        neg = reference_tiles(ex, queries, ndocs)
        pos_s, neg_s = m(torch.cat(list(tiles)), torch.cat(list(neg)))
        score = torch.cat([pos_s, neg_s])
        coef = torch.linspace(-1.0, 1.5, score.numel())
        (score * coef).sum().backward()
        out["neg_tiles"], out["score"], out["loss_coef"] = neg[:, 0].numpy(), score.detach().numpy(), coef.numpy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["grad." + k] = p.grad.numpy().copy()
    else:
        seen = {}
        h = m.DeepTileBar1.W1.register_forward_pre_hook(lambda mod, inp: seen.__setitem__("ev", inp[0].detach().clone()))
        with torch.no_grad():
            score = m.test_forward(torch.cat([batch["posdoc"][i] for i in range(len(batch["qid"]))]))
        h.remove()
        out["score"], out["evidence"] = score.numpy(), seen["ev"].numpy()
        s = out["score"]
        print(f"{name}: scores {np.round(s, 4)}; spread {s.max() - s.min():.4g}; tiles tf max {tiles[..., 0].max():.0f}, sim max "
              f"{tiles[..., -1].max():.7f}, sim min over live tiles {tiles[..., -1][tiles[..., -1] > 0].min():.3g}")
    np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)


def main():
    DTE, DTB = load_reference_deeptile()
    names = sys.argv[1:] or list(deeptile_case.CASES)
    unknown = [n for n in names if n not in deeptile_case.CASES]
    if unknown:
        raise SystemExit(f"unknown case(s) {unknown}; known: {list(deeptile_case.CASES)}")
    for name in names:
        gen(name, DTE, DTB)


if __name__ == "__main__":
    main()
