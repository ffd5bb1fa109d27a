"""CDSSM (reranker `CDSSM`) on the MI355X: capamd_cdssm_tower and capamd_cos_sigmoid_pairs (csrc/dssm.hip) against the float64
restatement on the same inputs and against the reference's fixtures (tests/golden/cdssm_*.npz), their invariances, and the serving paths.

The tolerance is not a constant.  The yardstick is the reference's own fp32 error on a case, e_ref = max |fixture - float64 restatement|
per output (scores; each tower's output); the kernels sum the taps in another order than ATen's convolution, so they get
max(4 e_ref, 16 fp32 ulp of the output's scale), as tests/test_gpu_hint.py does.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from capreolus_amd.reranker import CDSSM
from tests import cdssm_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _plugin(name):
    r, m = cdssm_case.build(name, CDSSM)
    m.to(DEV).eval()
    return r, m


def _batch(q, d):
    return {"query": torch.from_numpy(q).to(DEV), "posdoc": torch.from_numpy(d).to(DEV), "query_idf": torch.zeros(q.shape, device=DEV)}


def _f64(m, q, d):
    """the float64 restatement on the host: (scores [B], query tower [B, R], document tower [B, R])"""
    with torch.no_grad():
        return tuple(t.numpy() for t in m._forward_aten(torch.from_numpy(d), torch.from_numpy(q), dtype=torch.float64, return_towers=True))


def _bound(e_ref, scale):
    return max(4.0 * e_ref, 16.0 * float(np.spacing(np.float32(scale))))


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """(float64 scores and towers, e_ref of each) of a fixture - computed once, shared, left alone"""
    c = cdssm_case.load(name)
    want = _f64(cdssm_case.build(name, CDSSM)[1].eval(), c["query"], c["posdoc"])
    return want, tuple(float(np.abs(c[k] - w).max()) for k, w in zip(("score", "qtower", "dtower"), want))


def _compare(label, got, want, e_refs):
    """prints every figure, then asserts scores and both towers against float64 within the bound"""
    lines, ok = [], True
    for what, g, w, e in zip(("scores", "query tower", "document tower"), got, want, e_refs):
        scale = max(float(np.abs(w).max()), float(np.finfo(np.float32).tiny))
        err, b = float(np.abs(g - w).max()), _bound(e, scale)
        lines.append(f"{what} e_ref {e:.3g} err {err:.3g} bound {b:.3g} scale {scale:.3g}")
        ok = ok and np.all(np.isfinite(g)) and err <= b
    print(f"\n{label}: " + "; ".join(lines))
    assert ok, lines


@pytest.mark.parametrize("name", cdssm_case.SCORE_CASES)
def test_scores_and_towers_against_float64_and_the_reference(name):
    c = cdssm_case.load(name)
    want, e_refs = _yardstick(name)
    r, m = _plugin(name)
    b = _batch(c["query"], c["posdoc"])
    with torch.no_grad():
        score, qt, dt = m.forward_engine(b["posdoc"], b["query"], towers=True)
        test = r.test(b)
    assert torch.equal(test, score) and test.dtype == torch.float32
    got = (score.cpu().numpy(), qt.cpu().numpy(), dt.cpu().numpy())
    _compare(name, got, want, e_refs)
    err_fix, b_s = float(np.abs(got[0] - c["score"]).max()), _bound(e_refs[0], np.abs(want[0]).max())
    print(f"{name}: kernel-vs-fixture {err_fix:.3g} bound {b_s:.3g}")
    assert err_fix <= b_s, (err_fix, b_s)
    if name == "cdssm_negbias":
        assert got[0][-1] == 0.5 and not got[2][-1].any()          # the all-pad document: an all-zero representation, exactly 0.5


@pytest.mark.parametrize("point", cdssm_case.SWEEP, ids=lambda p: cdssm_case.sweep_key(*p))
def test_every_length_and_geometry_against_float64(point):
    """cdssm_case.sweep_case: a random row, one with a padded tail, one of pads, on a table whose row 0 is not zero.  e_ref is the
    reference's own error at this point (tests/golden/cdssm_sweep.npz against the float64 restatement)"""
    cfg, ex, w, q, d = cdssm_case.sweep_case(*point)
    z, key = cdssm_case.load("cdssm_sweep"), cdssm_case.sweep_key(*point)
    want = _f64(cdssm_case.build_from(cfg, ex, w, CDSSM)[1].eval(), q, d)
    e_refs = tuple(float(np.abs(z[f"{k}.{key}"] - x).max()) for k, x in zip(("score", "qtower", "dtower"), want))
    r, m = cdssm_case.build_from(cfg, ex, w, CDSSM)
    m.to(DEV).eval()
    with torch.no_grad():
        got = m.forward_engine(torch.from_numpy(d).to(DEV), torch.from_numpy(q).to(DEV), towers=True)
    _compare("sweep " + key, tuple(t.cpu().numpy() for t in got), want, e_refs)


def test_scores_do_not_depend_on_batch_size_and_pairs_equal_repeated_rows():
    c = cdssm_case.load("cdssm_default")
    r, m = _plugin("cdssm_default")
    idx = np.arange(70) % c["query"].shape[0]
    q, d = c["query"][idx], c["posdoc"][idx]
    with torch.no_grad():
        s70 = r.test(_batch(q, d))
        s7 = r.test(_batch(q[:7], d[:7]))
        s1 = torch.cat([r.test(_batch(q[i:i + 1], d[i:i + 1])) for i in range(7)])
        assert torch.equal(s7, s70[:7]) and torch.equal(s1, s70[:7])
        assert torch.equal(s70[:6], s70[6:12]) and torch.equal(s70[:6], s70[60:66])
        # one query row against every document through the index arrays = that query repeated
        docs = torch.from_numpy(c["posdoc"]).to(DEV)
        n = docs.shape[0]
        one = torch.from_numpy(c["query"][2:3]).to(DEV)
        pairs = r.test_pairs(one, docs, torch.zeros(n, dtype=torch.int32, device=DEV), torch.arange(n, dtype=torch.int32, device=DEV))
        assert torch.equal(pairs, r.test({"query": one.expand(n, -1).contiguous(), "posdoc": docs}))
        # and in another order, with repeats
        pd = torch.tensor([5, 0, 0, 3], dtype=torch.int32, device=DEV)
        pq = torch.tensor([1, 4, 1, 1], dtype=torch.int32, device=DEV)
        qs = torch.from_numpy(c["query"]).to(DEV)
        assert torch.equal(r.test_pairs(qs, docs, pq, pd), r.test({"query": qs[pq.long()], "posdoc": docs[pd.long()]}))


def test_resident_and_predict_equal_test():
    from capreolus_amd.feeder import CandidateStore
    from capreolus_amd.trainer.pytorch import PytorchTrainer

    c = cdssm_case.load("cdssm_multiple")
    r, m = _plugin("cdssm_multiple")
    B = c["query"].shape[0]
    store = CandidateStore(DEV)
    for i in range(B):
        store.add_query(f"q{i}", c["query"][i], np.zeros(c["query"].shape[1], dtype=np.float32))
        store.add_doc(f"d{i}", c["posdoc"][i])
    store.finalize()
    pq = torch.arange(B, dtype=torch.int32, device=DEV)
    pd = torch.as_tensor([store.drow[f"d{i}"] for i in range(B)], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        want = r.test(_batch(c["query"], c["posdoc"]))
        assert torch.equal(r.test_resident(store, pq, pd), want)
    q2d = {f"q{i}": [f"d{i}"] for i in range(B)}

    class Sampler(torch.utils.data.IterableDataset):
        qid_to_docids = q2d

        def __iter__(self):
            for i in range(B):
                yield {"qid": f"q{i}", "posdocid": f"d{i}", "query": c["query"][i], "posdoc": c["posdoc"][i],
                       "query_idf": np.zeros(c["query"].shape[1], dtype=np.float32)}

        def __len__(self):
            return B

        def get_qid_docid_pairs(self):
            return ((q, d) for q, ds in self.qid_to_docids.items() for d in ds)

    preds = PytorchTrainer({"batch": 2}).predict(r, Sampler())
    direct = want.cpu().numpy().astype(np.float16)
    for i in range(B):
        assert preds[f"q{i}"][f"d{i}"] == float(direct[i]), i


def test_out_of_range_ids_raise_and_the_next_call_is_clean():
    c = cdssm_case.load("cdssm_multiple")
    r, m = _plugin("cdssm_multiple")
    with torch.no_grad():
        want = r.test(_batch(c["query"], c["posdoc"]))
        for key, bad in (("posdoc", 10 ** 6), ("query", 64), ("posdoc", -1)):
            b = _batch(c["query"], c["posdoc"])
            b[key][0, 1] = bad
            with pytest.raises(IndexError):
                r.test(b)
            assert torch.equal(r.test(_batch(c["query"], c["posdoc"])), want)


def test_score_in_training_mode_runs_the_restatement_with_gradients():
    c = cdssm_case.load("cdssm_grad")
    r, m = _plugin("cdssm_grad")
    assert r.config["dropoutrate"] == 0
    m.train()
    b = _batch(c["query"], c["posdoc"])
    b["negdoc"] = torch.from_numpy(c["negdoc"]).to(DEV)
    pos, neg = r.score(b)
    assert pos.requires_grad and neg.requires_grad and pos.shape == neg.shape == (c["query"].shape[0],)
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().cpu().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"]).to(DEV)).sum().backward()
    for k in ("conv.0.weight", "conv.0.bias"):
        g, want = dict(m.named_parameters())[k].grad.cpu().numpy(), c["grad." + k]
        assert np.abs(g - want).max() <= 1e-4 * np.abs(want).max(), k
