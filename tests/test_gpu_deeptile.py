"""DeepTileBar (reranker `DeepTileBar`) on the MI355X: capamd_deeptile_forward and capamd_deeptile_color (csrc/deeptile.hip) against the
float64 restatements on the same inputs and against the reference's fixtures (tests/golden/deeptile_*.npz), their invariances, refusals
and the serving path.

The tolerance is not a constant.  The yardstick is the reference's own fp32 error on a case, e_ref = max |fixture - float64 restatement|
per output (scores; W1 input; sim channel); the kernels get max(4 e_ref, 16 fp32 ulp of the output's scale).  The integer-valued channels
(tf, and idf, which is copied) are exact.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

from capreolus_amd import deeptiles, engine
from capreolus_amd.reranker import DeepTileBar
from tests import deeptile_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _plugin(name):
    r, m = deeptile_case.build(name, DeepTileBar)
    m.to(DEV).eval()
    return r, m


def _bound(e_ref, scale):
    return max(4.0 * e_ref, 16.0 * float(np.spacing(np.float32(scale))))


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """(float64 scores, float64 W1 input [B, 10, H], their e_ref, float64 tiles, e_ref of sim) of a fixture - computed once, shared, left
    alone"""
    c = deeptile_case.load(name)
    m = deeptile_case.build(name, DeepTileBar)[1].eval()
    with torch.no_grad():
        s64, ev64 = m._forward_aten(torch.from_numpy(c["tiles"]), dtype=torch.float64, return_evidence=True)
    s64, ev64 = s64.numpy(), ev64.numpy()
    t64 = deeptiles.color_numpy(c["query"], c["posdoc"], c["posdoc_segments"], c["query_idf"], deeptile_case.embeddings(name), deeptile_case.CASES[name]["C"])
    return (s64, ev64, float(np.abs(c["score"] - s64).max()), float(np.abs(c["evidence"].reshape(ev64.shape) - ev64).max()), t64,
            float(np.abs(c["tiles"][..., -1] - t64[..., -1]).max()))


def _id_batch(c):
    return {"query": torch.from_numpy(c["query"]).to(DEV), "query_idf": torch.from_numpy(c["query_idf"]).to(DEV),
            "posdoc": torch.from_numpy(c["posdoc"]).to(DEV), "posdoc_segments": torch.from_numpy(c["posdoc_segments"]).to(DEV)}


@pytest.mark.parametrize("name", deeptile_case.SCORE_CASES)
def test_scores_and_evidence_against_float64_and_the_reference(name):
    c = deeptile_case.load(name)
    s64, ev64, e_s, e_ev, _, _ = _yardstick(name)
    r, m = _plugin(name)
    tiles = torch.from_numpy(c["tiles"]).to(DEV)
    with torch.no_grad():
        score, ev = m.forward_engine(tiles, evidence=True)
        test = r.test({"qid": list(range(len(tiles))), "posdoc": tiles[:, None]})       # the reference's input: a batch of [1, Q, P, C] tiles
    assert torch.equal(test, score) and test.dtype == torch.float32 and ev.shape == ev64.shape
    score, ev = score.cpu().numpy(), ev.cpu().numpy()
    s_scale, ev_scale = np.abs(s64).max(), np.abs(ev64).max()
    b_s, b_ev = _bound(e_s, s_scale), _bound(e_ev, ev_scale)
    err_s, err_ev, err_fix = np.abs(score - s64).max(), np.abs(ev - ev64).max(), np.abs(score - c["score"]).max()
    err_evfix = np.abs(ev - c["evidence"].reshape(ev.shape)).max()
    print(f"\n{name}: scores e_ref {e_s:.3g} bound {b_s:.3g} kernel-vs-f64 {err_s:.3g} kernel-vs-fixture {err_fix:.3g} scale {s_scale:.3g}; "
          f"W1 input e_ref {e_ev:.3g} bound {b_ev:.3g} kernel-vs-f64 {err_ev:.3g} kernel-vs-fixture {err_evfix:.3g} scale {ev_scale:.3g}")
    assert np.all(np.isfinite(score)) and np.all(np.isfinite(ev))
    assert err_ev <= b_ev, (err_ev, b_ev)
    assert err_evfix <= b_ev, (err_evfix, b_ev)
    assert err_s <= b_s, (err_s, b_s)
    assert err_fix <= b_s, (err_fix, b_s)


@pytest.mark.parametrize("name", list(deeptile_case.CASES))
def test_coloured_tiles_against_float64_and_the_reference(name):
    c = deeptile_case.load(name)
    t64, e_sim = _yardstick(name)[4:] if name in deeptile_case.SCORE_CASES else (None, None)
    if t64 is None:
        t64 = deeptiles.color_numpy(c["query"], c["posdoc"], c["posdoc_segments"], c["query_idf"], deeptile_case.embeddings(name), deeptile_case.CASES[name]["C"])
        e_sim = float(np.abs(c["tiles"][..., -1] - t64[..., -1]).max())
    b = _id_batch(c)
    emb = torch.from_numpy(deeptile_case.embeddings(name)).to(DEV)
    tiles = deeptiles.color(b["query"], b["posdoc"], b["posdoc_segments"], b["query_idf"], emb, deeptile_case.CASES[name]["C"]).cpu().numpy()
    assert tiles.shape == c["tiles"].shape and tiles.dtype == np.float32
    np.testing.assert_array_equal(tiles[..., :-1], c["tiles"][..., :-1])                 # tf and idf: exactly the reference's
    bound = _bound(e_sim, 1.0)
    err, err_fix = np.abs(tiles[..., -1] - t64[..., -1]).max(), np.abs(tiles[..., -1] - c["tiles"][..., -1]).max()
    near = (t64[..., -1] > 0.999) & (t64[..., -1] < 1.0)
    print(f"\n{name}: sim e_ref {e_sim:.3g} bound {bound:.3g} kernel-vs-f64 {err:.3g} kernel-vs-fixture {err_fix:.3g}; "
          f"{int(near.sum())} tiles near 1, kernel-vs-f64 there {np.abs(tiles[..., -1] - t64[..., -1])[near].max():.3g}")
    assert near.any() and err <= bound and err_fix <= bound, (err, err_fix, bound)
    assert (tiles[..., -1][c["tiles"][..., -1] == 0] == 0).all()                          # pad terms, pad segments, literal pad tokens: exactly 0


@pytest.mark.parametrize("name", ("deeptile_default", "deeptile_notf", "deeptile_wide"))
def test_test_ids_equals_test_on_the_coloured_tiles(name):
    c = deeptile_case.load(name)
    r, m = _plugin(name)
    b = _id_batch(c)
    with torch.no_grad():
        tiles = r.color(b)
        from_ids = r.test_ids(b)
        from_tiles = r.test({"posdoc": tiles[:, None]})
    assert torch.equal(from_ids, from_tiles) and from_ids.shape == (c["query"].shape[0],)
    s64, _, e_s, _, _, _ = _yardstick(name)
    # (the tiles differ from the reference's by the colouring's error, so this is looser than bit equality and not the kernel's bound: a sanity figure)
    print(f"\n{name}: scores from ids vs float64 on the reference's tiles {np.abs(from_ids.cpu().numpy() - s64).max():.3g} (e_ref {e_s:.3g})")


def test_scores_do_not_depend_on_the_batch():
    """seventy rows repeating six documents equal the six scored one by one, bitwise - scores and coloured tiles"""
    a = deeptile_case.load("deeptile_default")
    r, m = _plugin("deeptile_default")
    six = torch.from_numpy(np.concatenate([a["tiles"], a["tiles"][:1] * 0.5])).to(DEV)
    idx = torch.arange(70, device=DEV) % 6
    with torch.no_grad():
        s70 = r.test({"posdoc": six[idx][:, None]})
        s1 = torch.cat([r.test({"posdoc": six[i:i + 1][:, None]}) for i in range(6)])
    assert torch.equal(s70[:6], s1) and torch.equal(s70, s1[idx])
    ids = _id_batch(a)
    emb = torch.from_numpy(deeptile_case.embeddings("deeptile_default")).to(DEV)
    rows = torch.arange(70, device=DEV) % 5
    t70 = deeptiles.color(*(ids[k][rows] for k in ("query", "posdoc", "posdoc_segments", "query_idf")), emb)
    t1 = torch.cat([deeptiles.color(*(ids[k][i:i + 1] for k in ("query", "posdoc", "posdoc_segments", "query_idf")), emb) for i in range(5)])
    assert torch.equal(t70, t1[rows])


def test_an_id_outside_the_table_raises():
    c = deeptile_case.load("deeptile_default")
    r, m = _plugin("deeptile_default")
    b = _id_batch(c)
    b["posdoc"][0, 1] = 10 ** 6
    with torch.no_grad(), pytest.raises(engine.IdRangeError):
        r.test_ids(b)
    b = _id_batch(c)
    b["query"][0, 1] = deeptile_case.V
    with torch.no_grad(), pytest.raises(engine.IdRangeError):
        r.test_ids(b)
    b = _id_batch(c)
    b["posdoc"][0, int(c["posdoc_segments"][0, -1])] = 10 ** 6        # behind the last offset: never read
    with torch.no_grad():
        assert torch.isfinite(r.test_ids(b)).all()


def test_a_decreasing_offset_is_clamped_and_reported():
    c = deeptile_case.load("deeptile_default")
    b = _id_batch(c)
    emb = torch.from_numpy(deeptile_case.embeddings("deeptile_default")).to(DEV)
    args = lambda: (b["query"], b["posdoc"], b["posdoc_segments"], b["query_idf"], emb)      # noqa: E731
    good = deeptiles.color(*args())
    L = c["posdoc"].shape[1]
    for p, v in ((3, 0), (5, -7), (20, L + 50), (0, 2 * L)):
        b["posdoc_segments"] = torch.from_numpy(c["posdoc_segments"].copy()).to(DEV)
        b["posdoc_segments"][1, p] = v
        with pytest.raises(ValueError, match="segment offset"):
            deeptiles.color(*args())
        tiles = deeptiles.color(*args(), check=False)                  # the clamped result, the bit left in the status word
        st = engine.status_word(tiles.device)
        assert int(st.t.item()) == 128
        st.t.zero_()
        assert torch.isfinite(tiles).all() and torch.equal(tiles[0], good[0]) and torch.equal(tiles[2:], good[2:])
    b["posdoc_segments"] = torch.from_numpy(c["posdoc_segments"]).to(DEV)
    assert torch.equal(deeptiles.color(*args()), good)


def test_predict_equals_test():
    """PytorchTrainer.predict takes a reranker that is not resident as it is: the sampler yields the reference's [1, Q, P, C] tile tensors"""
    from capreolus_amd.trainer.pytorch import PytorchTrainer

    c = deeptile_case.load("deeptile_default")
    r, m = _plugin("deeptile_default")
    B = c["tiles"].shape[0]
    with torch.no_grad():
        want = r.test({"posdoc": torch.from_numpy(c["tiles"]).to(DEV)[:, None]})
    q2d = {f"q{i}": [f"d{i}"] for i in range(B)}

    class Sampler(torch.utils.data.IterableDataset):
        qid_to_docids = q2d

        def __iter__(self):
            for i in range(B):
                yield {"qid": f"q{i}", "posdocid": f"d{i}", "posdoc": torch.from_numpy(c["tiles"][i:i + 1]),
                       "query_idf": np.zeros(c["query"].shape[1], dtype=np.float32)}

        def __len__(self):
            return B

        def get_qid_docid_pairs(self):
            return ((q, d) for q, ds in self.qid_to_docids.items() for d in ds)

    preds = PytorchTrainer({"batch": 2}).predict(r, Sampler())
    direct = want.cpu().numpy().astype(np.float16)
    for i in range(B):
        assert preds[f"q{i}"][f"d{i}"] == float(direct[i]), i


def test_score_in_training_mode_runs_the_restatement_with_gradients():
    c = deeptile_case.load("deeptile_grad")
    r, m = _plugin("deeptile_grad")
    m.train()
    pos, neg = r.score({"posdoc": torch.from_numpy(c["tiles"]).to(DEV)[:, None], "negdoc": torch.from_numpy(c["neg_tiles"]).to(DEV)[:, None]})
    assert pos.requires_grad and neg.requires_grad and pos.shape == neg.shape == (c["tiles"].shape[0],)
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().cpu().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"]).to(DEV)).sum().backward()
    for k in ("DeepTileBar1.conv10.weight", "DeepTileBar1.lstm1.weight_hh_l0", "DeepTileBar1.W1.weight", "DeepTileBar1.W3.bias"):
        g, want = dict(m.named_parameters())[k].grad.cpu().numpy(), c["grad." + k]
        assert np.abs(g - want).max() <= 1e-4 * np.abs(want).max(), k
