"""TK (reranker `TK`) on the MI355X: capamd_tk_forward (csrc/tk.hip) against the reference's fixtures (tests/golden/tk_*.npz) and
against the float64 restatement on the device, its invariances (micro-batch size, batch composition), and the serving paths."""
import numpy as np
import pytest
import torch

from capreolus_amd.reranker import TK
from tests import tk_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
# features: |got - want| <= REL x the largest feature magnitude of the pair (fp32 end to end against the reference's fp32 on the host)
REL = 1e-5


def _plugin(name):
    r, m = tk_case.build(name, TK)
    m.to(DEV).eval()
    return r, m


def _batch(c, sl=slice(None)):
    return {"query": torch.from_numpy(c["query"][sl]).to(DEV), "posdoc": torch.from_numpy(c["posdoc"][sl]).to(DEV),
            "query_idf": torch.zeros(c["query"][sl].shape, device=DEV)}


def _check_features(got, want, rel=REL):
    scale = np.abs(want).max(axis=1, keepdims=True)
    err = np.abs(got - want)
    assert np.all(err <= rel * scale), (err / scale).max()


@pytest.mark.parametrize("name", tk_case.SCORE_CASES)
def test_features_and_scores_match_the_reference(name):
    c = tk_case.load(name)
    r, m = _plugin(name)
    with torch.no_grad():
        score, feats = m.forward_engine(_batch(c)["posdoc"], _batch(c)["query"], features=True)
        test = r.test(_batch(c))
    score, feats = score.cpu().numpy(), feats.cpu().numpy()
    assert torch.equal(test.cpu(), torch.from_numpy(score))
    _check_features(feats, np.concatenate([c["s_log_k"], c["s_len_k"]], axis=1))
    # the score is a fixed linear map of the features: its bound follows from theirs
    w = np.abs(np.concatenate([m.s_log_fcc.weight.detach().cpu().numpy()[0] * abs(float(m.comb_fcc.weight[0, 0].detach())),
                               m.s_len_fcc.weight.detach().cpu().numpy()[0] * abs(float(m.comb_fcc.weight[0, 1].detach()))]))
    bound = REL * np.abs(np.concatenate([c["s_log_k"], c["s_len_k"]], axis=1)).max(axis=1) * w.sum() * 1.01
    assert np.all(np.abs(score - c["score"]) <= bound), np.abs(score - c["score"]) / bound
    # rank order equals the reference's wherever the reference's gap exceeds twice the bound
    ref = c["score"].astype(np.float64)
    for i in range(len(ref)):
        for j in range(len(ref)):
            if ref[i] - ref[j] > bound[i] + bound[j]:
                assert score[i] > score[j], (i, j)


@pytest.mark.parametrize("name", tk_case.SCORE_CASES)
def test_against_float64_on_the_device(name):
    """every kernel at once against the float64 restatement on the device: padded head slots and widths (D = 300 -> 320, 50 -> 64,
    head width 30 / 50 / 10 -> slot 32 / 64 / 16), LayerNorm over the real columns, the masked attention including rows that attend
    to nothing (the all-pad document and the zero-row token under usemask), the pooling with its closed-form pads"""
    c = tk_case.load(name)
    r, m = _plugin(name)
    b = _batch(c)
    with torch.no_grad():
        _, feats = m.forward_engine(b["posdoc"], b["query"], features=True)
        m64 = tk_case.build(name, TK)[1].double().to(DEV).eval()
        s64, f64 = m64._forward_aten(b["posdoc"], b["query"], return_features=True)
    _check_features(feats.cpu().numpy(), f64.cpu().numpy())
    assert torch.isfinite(s64).all()


@pytest.mark.parametrize("name", tk_case.SCORE_CASES)
def test_scores_do_not_depend_on_microbatch_or_batch_composition(name):
    c = tk_case.load(name)
    r, m = _plugin(name)
    b = _batch(c)
    B = c["query"].shape[0]
    with torch.no_grad():
        want = r.test(b)
        for nb in (1, 2, 3, B):
            m._engine.docs_per_microbatch = nb
            assert torch.equal(r.test(b), want), nb
        m._engine.docs_per_microbatch = None
        split = torch.cat([r.test(_batch(c, slice(0, 3))), r.test(_batch(c, slice(3, None)))])
        assert torch.equal(split, want)
        perm = torch.randperm(B, device=DEV)
        assert torch.equal(r.test({k: v[perm] for k, v in b.items()}), want[perm])


def test_large_call_matches_small_calls():
    """1000 candidates of the default geometry in one call (several micro-batches) equal the same documents scored 8 at a time"""
    c = tk_case.load("tk_default")
    r, m = _plugin("tk_default")
    g = torch.Generator().manual_seed(5)
    B = 1000
    q = torch.from_numpy(c["query"][0:1]).repeat(B, 1).to(DEV)
    d = torch.randint(0, 400, (B, 800), generator=g).to(DEV)
    d[::7, 500:] = 0
    with torch.no_grad():
        m._engine.docs_per_microbatch = 300
        big = m.forward_engine(d, q)
        m._engine.docs_per_microbatch = None
        small = torch.cat([m.forward_engine(d[i:i + 8], q[i:i + 8]) for i in (0, 296, 992)])
    idx = torch.cat([torch.arange(0, 8), torch.arange(296, 304), torch.arange(992, 1000)]).to(DEV)
    assert torch.equal(big[idx], small)
    assert torch.isfinite(big).all()


def test_resident_and_predict_equal_test():
    from capreolus_amd.feeder import CandidateStore
    from capreolus_amd.trainer.pytorch import PytorchTrainer

    c = tk_case.load("tk_small")
    r, m = _plugin("tk_small")
    B = c["query"].shape[0]
    store = CandidateStore(DEV)
    for i in range(B):
        store.add_query(f"q{i}", c["query"][i], np.zeros(c["query"].shape[1], dtype=np.float32))
        store.add_doc(f"d{i}", c["posdoc"][i])
    store.finalize()
    pq = torch.arange(B, dtype=torch.int32, device=DEV)
    pd = torch.as_tensor([store.drow[f"d{i}"] for i in range(B)], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        want = r.test(_batch(c))
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


def test_out_of_range_ids_raise():
    c = tk_case.load("tk_small")
    r, m = _plugin("tk_small")
    b = _batch(c)
    b["posdoc"] = b["posdoc"].clone()
    b["posdoc"][0, 5] = 10 ** 6
    with torch.no_grad(), pytest.raises(IndexError):
        r.test(b)
    with torch.no_grad():
        assert torch.isfinite(r.test(_batch(c))).all()


def test_training_mode_runs_the_restatement_on_the_device():
    c = tk_case.load("tk_grad")
    r, m = _plugin("tk_grad")
    m.train()
    m.position_encoder.dropout.p = 0.0
    b = _batch(c)
    score = m(b["posdoc"], b["query"], None).view(-1)
    np.testing.assert_allclose(score.detach().cpu().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"]).to(DEV)).sum().backward()
    g = m.transformer_encoder.layers[0].self_attn.in_proj_weight.grad.cpu().numpy()
    want = c["grad.transformer_encoder.layers.0.self_attn.in_proj_weight"]
    assert np.abs(g - want).max() <= 1e-4 * np.abs(want).max()
