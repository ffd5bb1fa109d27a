"""DSSM (reranker `DSSM`) on the MI355X: capamd_dssm_tower and capamd_cos_sigmoid_pairs (csrc/dssm.hip) against the float64 restatement
on the same inputs and against the reference's fixtures (tests/golden/dssm_*.npz), their invariances, the two input routes, and predict.

The tolerance is not a constant.  The yardstick is the reference's own fp32 error on a case, e_ref = max |fixture - float64 restatement|
per output (scores; each tower's output); the kernels sum a bag's entries in another order than ATen's matrix product over the dense
row, so they get max(4 e_ref, 16 fp32 ulp of the output's scale), as tests/test_gpu_hint.py does.  Every figure is printed before it
is asserted."""
import functools

import numpy as np
import pytest
import torch

from capreolus_amd import bags
from capreolus_amd.reranker import DSSM
from tests import dssm_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _plugin(name):
    r, m = dssm_case.build(name, DSSM)
    m.to(DEV).eval()
    return r, m


def _batch(c, rows=None):
    q, d = dssm_case.bags_of(c, "query"), dssm_case.bags_of(c, "posdoc")
    if rows is not None:
        q, d = _take(q, rows), _take(d, rows)
    return {"query": q.to(DEV), "posdoc": d.to(DEV), "query_idf": torch.zeros(q.rows, 4, device=DEV)}


def _take(b, rows):
    """the bags of `rows` (any order, repeats allowed) as new Bags"""
    parts = [(b.idx[b.indptr[n]:b.indptr[n + 1]], b.val[b.indptr[n]:b.indptr[n + 1]]) for n in rows]
    indptr = torch.tensor([0] + list(np.cumsum([len(i) for i, _ in parts])), dtype=torch.int64)
    return bags.Bags(indptr, torch.cat([i for i, _ in parts]), torch.cat([v for _, v in parts]))


def _bound(e_ref, scale):
    return max(4.0 * e_ref, 16.0 * float(np.spacing(np.float32(scale))))


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """(float64 scores and towers, e_ref of each) of a fixture - computed once, shared, left alone"""
    c = dssm_case.load(name)
    m = dssm_case.build(name, DSSM)[1].eval()
    with torch.no_grad():
        want = tuple(t.numpy() for t in m._forward_aten(dssm_case.bags_of(c, "posdoc"), dssm_case.bags_of(c, "query"), dtype=torch.float64,
                                                        return_towers=True))
    return want, tuple(float(np.abs(c[k] - w).max()) for k, w in zip(("score", "qtower", "dtower"), want))


@pytest.mark.parametrize("name", dssm_case.SCORE_CASES)
def test_scores_and_towers_against_float64_and_the_reference(name):
    c = dssm_case.load(name)
    want, e_refs = _yardstick(name)
    r, m = _plugin(name)
    b = _batch(c)
    with torch.no_grad():
        score, qt, dt = m.forward_engine(b["posdoc"], b["query"], towers=True)
        test = r.test(b)
    assert torch.equal(test, score) and test.dtype == torch.float32
    got = (score.cpu().numpy(), qt.cpu().numpy(), dt.cpu().numpy())
    lines, ok = [], True
    for what, g, w, e in zip(("scores", "query tower", "document tower"), got, want, e_refs):
        scale = float(np.abs(w).max())
        err, bd = float(np.abs(g - w).max()), _bound(e, scale)
        lines.append(f"{what} e_ref {e:.3g} err {err:.3g} bound {bd:.3g} scale {scale:.3g}")
        ok = ok and np.all(np.isfinite(g)) and err <= bd
    err_fix, b_s = float(np.abs(got[0] - c["score"]).max()), _bound(e_refs[0], np.abs(want[0]).max())
    print(f"\n{name}: " + "; ".join(lines) + f"; kernel-vs-fixture {err_fix:.3g}")
    assert ok, lines
    assert err_fix <= b_s, (err_fix, b_s)


def test_an_empty_bag_is_relu_of_the_bias_through_the_later_layers():
    c = dssm_case.load("dssm_two")
    r, m = _plugin("dssm_two")
    b = _batch(c)
    with torch.no_grad():
        _, _, dt = m.forward_engine(b["posdoc"], b["query"], towers=True)
        h = torch.relu(m.ffw.linear0.bias.double())
        h = torch.relu(torch.nn.functional.linear(h, m.ffw.linear1.weight.double(), m.ffw.linear1.bias.double()))
    err = float((dt[-1].double() - h).abs().max())
    print(f"\nempty bag: err {err:.3g} scale {float(h.abs().max()):.3g}")
    assert err <= 16.0 * float(np.spacing(np.float32(h.abs().max().item())))


def test_dense_route_equals_bags_route_and_scores_do_not_depend_on_batch_size():
    c = dssm_case.load("dssm_default")
    r, m = _plugin("dssm_default")
    nvocab = int(c["nvocab"])
    rows = list(np.arange(70) % 6)
    with torch.no_grad():
        b70 = _batch(c, rows)
        s70 = r.test(b70)
        dense = {"query": b70["query"].to_dense(nvocab), "posdoc": b70["posdoc"].to_dense(nvocab), "query_idf": b70["query_idf"]}
        assert torch.equal(r.test(dense), s70)
        assert torch.equal(r.test({k: (v.double() if k != "query_idf" else v) for k, v in dense.items()}), s70)     # (counts in any dtype)
        s7 = r.test(_batch(c, rows[:7]))
        s1 = torch.cat([r.test(_batch(c, rows[i:i + 1])) for i in range(7)])
        assert torch.equal(s7, s70[:7]) and torch.equal(s1, s70[:7])
        assert torch.equal(s70[:6], s70[6:12]) and torch.equal(s70[:6], s70[60:66])
        # one query bag against every document through the index arrays = that query repeated
        full = _batch(c)
        one = _take(dssm_case.bags_of(c, "query"), [2]).to(DEV)
        pairs = r.test_pairs(one, full["posdoc"], torch.zeros(6, dtype=torch.int32, device=DEV), torch.arange(6, dtype=torch.int32, device=DEV))
        assert torch.equal(pairs, r.test({"query": _take(dssm_case.bags_of(c, "query"), [2] * 6).to(DEV), "posdoc": full["posdoc"]}))


def test_the_long_bag_does_not_depend_on_its_neighbours():
    c = dssm_case.load("dssm_big")
    r, m = _plugin("dssm_big")
    d = dssm_case.bags_of(c, "posdoc")
    assert int(d.indptr[3] - d.indptr[2]) >= 3000
    lin = m._linears()
    with torch.no_grad():
        every = m._engine.tower(d.to(DEV), lin, 1)
        alone = m._engine.tower(_take(d, [2]).to(DEV), lin, 1)
        moved = m._engine.tower(_take(d, [5, 5, 2, 0]).to(DEV), lin, 1)
    assert torch.equal(alone[0], every[2]) and torch.equal(moved[2], every[2]) and torch.equal(moved[3], every[0])


def test_predict_equals_test():
    from capreolus_amd.trainer.pytorch import PytorchTrainer

    c = dssm_case.load("dssm_default")
    r, m = _plugin("dssm_default")
    nvocab, B = int(c["nvocab"]), 6
    q, d = dssm_case.bags_of(c, "query").to_dense(nvocab).numpy(), dssm_case.bags_of(c, "posdoc").to_dense(nvocab).numpy()
    with torch.no_grad():
        want = r.test(_batch(c))
    q2d = {f"q{i}": [f"d{i}"] for i in range(B)}

    class Sampler(torch.utils.data.IterableDataset):
        qid_to_docids = q2d

        def __iter__(self):
            for i in range(B):
                yield {"qid": f"q{i}", "posdocid": f"d{i}", "query": q[i], "posdoc": d[i], "query_idf": np.zeros(4, dtype=np.float32)}

        def __len__(self):
            return B

        def get_qid_docid_pairs(self):
            return ((q, d) for q, ds in self.qid_to_docids.items() for d in ds)

    preds = PytorchTrainer({"batch": 4}).predict(r, Sampler())
    direct = want.cpu().numpy().astype(np.float16)
    for i in range(B):
        assert preds[f"q{i}"][f"d{i}"] == float(direct[i]), i


def test_an_index_out_of_range_raises_and_the_next_call_is_clean():
    c = dssm_case.load("dssm_default")
    r, m = _plugin("dssm_default")
    with torch.no_grad():
        want = r.test(_batch(c))
        for key, bad in (("posdoc", 500), ("query", -1)):
            b = _batch(c)
            b[key].idx[1] = bad
            with pytest.raises(IndexError):
                r.test(b)
            assert torch.equal(r.test(_batch(c)), want)


def test_a_decreasing_indptr_raises_and_reads_nothing_out_of_bounds():
    """the arrays are exactly sized torch.empty's: a read outside them is a read outside the allocation's live bytes.  Bag 1's pair
    decreases (it is clamped to an empty bag) and bag 4's leaves [0, nnz]; the other bags' towers are unchanged"""
    c = dssm_case.load("dssm_default")
    r, m = _plugin("dssm_default")
    d = dssm_case.bags_of(c, "posdoc")
    lin = m._linears()
    with torch.no_grad():
        want = m._engine.tower(d.to(DEV), lin, 1)
        indptr, idx, val = (torch.empty(t.shape, dtype=t.dtype, device=DEV) for t in d)
        idx.copy_(d.idx)
        val.copy_(d.val)
        bad = d.indptr.clone()
        nnz = int(bad[-1])
        bad[2] = bad[1] - 3                       # bag 1 runs backwards; bag 2 then starts 3 entries early
        indptr.copy_(bad)
        with pytest.raises(ValueError, match="indptr"):
            m._engine.tower(bags.Bags(indptr, idx, val), lin, 1)
        got = m._engine.tower(bags.Bags(indptr, idx, val), lin, 1, check=False)
        from capreolus_amd import engine
        with pytest.raises(ValueError, match="indptr"):
            engine.status_word(got.device).raise_if_set()
        assert torch.equal(got[0], want[0]) and torch.equal(got[3:], want[3:])
        assert torch.equal(got[1], want[5])       # (clamped to an empty bag: document 5 of the fixture is the empty one)
        bad = d.indptr.clone()
        bad[5] = nnz + 10 ** 9                    # bag 4 would end, and bag 5 start, far outside the arrays
        indptr.copy_(bad)
        with pytest.raises(ValueError, match="indptr"):
            m._engine.tower(bags.Bags(indptr, idx, val), lin, 1)
        got = m._engine.tower(bags.Bags(indptr, idx, val), lin, 1, check=False)
        with pytest.raises(ValueError, match="indptr"):
            engine.status_word(got.device).raise_if_set()
        assert torch.equal(got[:4], want[:4]) and torch.isfinite(got).all()
        assert torch.equal(m._engine.tower(d.to(DEV), lin, 1), want)


def test_score_in_training_mode_runs_the_restatement_with_gradients():
    c = dssm_case.load("dssm_grad")
    r, m = _plugin("dssm_grad")
    m.train()
    for mod in m.ffw:
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0                           # dropout patched to the identity: the fixture's gradients are the function's
    nvocab = int(c["nvocab"])
    b = {k: dssm_case.bags_of(c, k).to(DEV).to_dense(nvocab) for k in ("query", "posdoc", "negdoc")}
    b["query_idf"] = torch.zeros(6, 4, device=DEV)
    pos, neg = r.score(b)
    assert pos.requires_grad and neg.requires_grad and pos.shape == neg.shape == (6,)
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().cpu().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"]).to(DEV)).sum().backward()
    for k, p in m.named_parameters():
        want = c["grad." + k]
        assert np.abs(p.grad.cpu().numpy() - want).max() <= 1e-4 * np.abs(want).max(), k
