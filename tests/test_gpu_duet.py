"""DUET (reranker `DUET`) on the MI355X: capamd_duet_forward (csrc/duet.hip) against the float64 restatement (tests/duet_case.restate) on
the same inputs and against the reference's fixtures (tests/golden/duet_*.npz), its invariances (batch size, micro-batch size, repetition),
its edge ids and its limits.

The tolerance is not a constant.  The yardstick is the reference's own fp32 error on a case, e_ref = max |fixture - float64| per output
(score, lm, dm, query vector, pooled map), computed from the fixture alone; the kernels sum in another order than ATen, so every output
gets max(4 e_ref, 16 fp32 ulp of its scale), as tests/test_gpu_hint.py does.  An output's scale is its largest magnitude over the case;
the score is the sum of two computed values and may cancel, so its scale is the largest |lm| + |dm|.  Every figure is printed before it is
asserted."""
import functools

import numpy as np
import pytest
import torch

from capreolus_amd import engine
from capreolus_amd.reranker import DUET
from tests import duet_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _plugin(name):
    r, m = duet_case.build(name, DUET)
    m.to(DEV).eval()
    return r, m


def _batch(q, d, idf):
    return {"query": torch.from_numpy(q).to(DEV), "posdoc": torch.from_numpy(d).to(DEV), "query_idf": torch.from_numpy(idf).to(DEV)}


def _engine(m, q, d, idf, check=True):
    """the five outputs of one capamd_duet_forward call, as numpy"""
    b = _batch(q, d, idf)
    with torch.no_grad():
        score, parts, qvec, pooled = m.forward_engine(b["posdoc"], b["query"], b["query_idf"], parts=True, evidence=True, check=check)
    parts = parts.cpu().numpy()
    return {"score": score.cpu().numpy(), "lm": parts[:, 0], "dm": parts[:, 1], "qvec": qvec.cpu().numpy(), "pooled": pooled.cpu().numpy()}


def _bound(e_ref, scale):
    return max(4.0 * e_ref, 16.0 * float(np.spacing(np.float32(scale))))


def _scales(want):
    tiny = float(np.finfo(np.float32).tiny)
    s = {k: max(float(np.abs(want[k]).max()), tiny) for k in duet_case.OUTPUTS}
    s["score"] = max(float((np.abs(want["lm"]) + np.abs(want["dm"])).max()), tiny)
    return s


def _e_refs(fixture, want, key=""):
    return {k: float(np.abs(fixture[k + key] - want[k]).max()) for k in duet_case.OUTPUTS}


def _compare(label, got, want, e_refs):
    """prints every figure, then asserts the five outputs against float64 within their bounds; returns the bounds"""
    scales, lines, ok, bounds = _scales(want), [], True, {}
    for k in duet_case.OUTPUTS:
        err, bounds[k] = float(np.abs(got[k] - want[k]).max()), _bound(e_refs[k], scales[k])
        lines.append(f"{k} e_ref {e_refs[k]:.3g} err {err:.3g} bound {bounds[k]:.3g} ratio {err / bounds[k]:.2f} scale {scales[k]:.3g}")
        ok = ok and got[k].shape == want[k].shape and bool(np.all(np.isfinite(got[k]))) and err <= bounds[k]
    print(f"\n{label}: " + "; ".join(lines))
    assert ok, lines
    return bounds


@functools.lru_cache(maxsize=None)
def _yardstick(name):
    """(float64 outputs, e_ref of each) of a fixture - computed once, shared, left alone"""
    c = duet_case.load(name)
    want = duet_case.restate(duet_case.config(name), duet_case.embeddings(name), duet_case.weights(name), c["query"], c["posdoc"], c["query_idf"])
    return want, _e_refs(c, want)


@pytest.mark.parametrize("name", duet_case.SCORE_CASES)
def test_outputs_against_float64_and_the_reference(name):
    c = duet_case.load(name)
    want, e_refs = _yardstick(name)
    r, m = _plugin(name)
    got = _engine(m, c["query"], c["posdoc"], c["query_idf"])
    with torch.no_grad():
        test = r.test(_batch(c["query"], c["posdoc"], c["query_idf"]))
    assert test.dtype == torch.float32 and np.array_equal(test.cpu().numpy(), got["score"])          # the plugin's test() IS the engine
    bounds = _compare(name, got, want, e_refs)
    err_fix = float(np.abs(got["score"] - c["score"]).max())
    print(f"{name}: kernel-vs-fixture {err_fix:.3g} bound {bounds['score']:.3g}")
    assert err_fix <= bounds["score"], (err_fix, bounds["score"])
    # the document of one term: its three convolution outputs carry through exactly the pooled positions whose window covers them
    L, s, p = c["posdoc"].shape[1], duet_case.single_position(c["posdoc"].shape[1]), got["pooled"]
    one, pads = p[duet_case.SINGLE], p[5]
    cover = np.zeros(L - 101, dtype=bool)
    cover[max(0, s - 101): s + 1] = True                                   # pooled position u covers the convolution positions u .. u + 99
    assert np.array_equal(one[:, ~cover], pads[:, ~cover])
    inner = one[:, max(0, s - 99): s - 1]                                  # ... all three of them: one value per filter
    assert inner.shape[1] > 0 and np.array_equal(inner, np.repeat(inner[:, :1], inner.shape[1], axis=1))
    assert np.array_equal(one[:, cover].max(axis=1), inner[:, 0])


def _sweep_point(point, B=3):
    cfg, ex, w, q, d, idf = duet_case.sweep_case(*point, B=B)
    z, key = duet_case.load("duet_sweep"), "." + duet_case.sweep_key(*point)
    want = duet_case.restate(cfg, ex.embeddings, w, q, d, idf)
    e_refs = _e_refs(z, want, key)
    r, m = duet_case.build_from(cfg, ex, w, DUET)
    m.to(DEV).eval()
    _compare("sweep" + key, _engine(m, q, d, idf), want, e_refs)


@pytest.mark.parametrize("point", duet_case.SWEEP, ids=lambda p: duet_case.sweep_key(*p))
def test_every_length_and_geometry_against_float64(point):
    """duet_case.sweep_case: a table whose row 0 is not zero; a document with a query term at both ends, one with a padded tail under a
    query with a pad, one of a single term.  e_ref is the reference's own error at this point (tests/golden/duet_sweep.npz)"""
    _sweep_point(point)


def test_the_sliding_maximum_and_the_sums_at_the_limits():
    """the largest L (8192: 32 tiles of pooled positions) with the largest nfilters (32) and lmhidden (256), random ids, two documents"""
    _sweep_point(duet_case.LIMITS, B=2)


def test_scores_do_not_depend_on_batch_microbatch_or_repetition():
    c = duet_case.load("duet_default")
    r, m = _plugin("duet_default")
    idx = np.arange(14) % c["query"].shape[0]
    q, d, idf = c["query"][idx], c["posdoc"][idx], c["query_idf"][idx]
    with torch.no_grad():
        s14 = r.test(_batch(q, d, idf))
        assert torch.equal(r.test(_batch(q, d, idf)), s14)                                           # a repeated call
        assert torch.equal(m.forward_engine(*(_batch(q, d, idf)[k] for k in ("posdoc", "query", "query_idf"))), s14)
        s1 = torch.cat([r.test(_batch(q[i:i + 1], d[i:i + 1], idf[i:i + 1])) for i in range(6)])     # batches of one
        assert torch.equal(s1, s14[:6]) and torch.equal(s14[:6], s14[6:12]) and torch.equal(s14[:2], s14[12:])
        assert m._engine.docs_per_microbatch is None
        for nb in (1, 2):
            m._engine.docs_per_microbatch = nb
            assert torch.equal(r.test(_batch(q, d, idf)), s14), nb
        m._engine.docs_per_microbatch = None


def test_pad_pad_matches_move_the_local_score_by_the_predicted_amount():
    """pair 1 of the fixture: a padded tail under a query whose last term is a pad with idf > 0.  Setting that idf to 0 removes the pads'
    columns; the local score moves by what float64 predicts"""
    name = "duet_default"
    c = duet_case.load(name)
    want, e_refs = _yardstick(name)
    idf0 = c["query_idf"].copy()
    idf0[1, 3] = 0.0
    want0 = duet_case.restate(duet_case.config(name), duet_case.embeddings(name), duet_case.weights(name), c["query"], c["posdoc"], idf0)
    r, m = _plugin(name)
    got, got0 = _engine(m, c["query"], c["posdoc"], c["query_idf"]), _engine(m, c["query"], c["posdoc"], idf0)
    move, predicted = float(got["lm"][1] - got0["lm"][1]), float(want["lm"][1] - want0["lm"][1])
    b = 2 * _bound(e_refs["lm"], _scales(want)["lm"])
    print(f"\npad-pad: lm moves by {move:.7g}, float64 predicts {predicted:.7g}, bound {b:.3g}")
    assert abs(predicted) > 1e-2 and abs(move - predicted) <= b
    assert np.array_equal(np.delete(got["lm"], 1), np.delete(got0["lm"], 1)) and np.array_equal(got["dm"], got0["dm"])


def test_out_of_range_ids_raise_or_score_as_zero_rows():
    name = "duet_padrow"
    c = duet_case.load(name)
    want, e_refs = _yardstick(name)
    r, m = _plugin(name)
    with torch.no_grad():
        clean = r.test(_batch(c["query"], c["posdoc"], c["query_idf"]))
        for key, row, col, bad in (("posdoc", 0, 7, 10 ** 6), ("query", 4, 1, 64), ("posdoc", 3, 209, -1)):
            b = _batch(c["query"], c["posdoc"], c["query_idf"])
            b[key][row, col] = bad
            with pytest.raises(IndexError):
                r.test(b)
            assert torch.equal(r.test(_batch(c["query"], c["posdoc"], c["query_idf"])), clean)
    # check=False: nothing raises, the bits stay in the status word, and the ids score as zero rows in the distributed model while the
    # local model still compares them as ids (the bad document id below equals the bad query id)
    q, d = c["query"].copy(), c["posdoc"].copy()
    q[0, 2] = d[0, 7] = d[0, 100] = 10 ** 6
    q[4, 0] = -5
    d[3, 209] = -1
    want_bad = duet_case.restate(duet_case.config(name), duet_case.embeddings(name), duet_case.weights(name), q, d, c["query_idf"])
    assert abs(want_bad["lm"][0] - want["lm"][0]) > 1e-3                       # the equal bad ids do match
    got = _engine(m, q, d, c["query_idf"], check=False)
    with pytest.raises(IndexError, match="document.*query"):
        engine.status_word(torch.device("cuda", torch.cuda.current_device())).raise_if_set()
    _compare(name + " with bad ids", got, want_bad, e_refs)


def test_entry_and_workspace_query_refuse_geometry_on_the_device():
    """the same refusals with live tensors: documents of another length than the model's, and a query of five terms"""
    c = duet_case.load("duet_min")
    r, m = _plugin("duet_min")
    b = _batch(c["query"], c["posdoc"], c["query_idf"])
    eng = m._engine
    with torch.no_grad():
        with pytest.raises(ValueError, match="unsupported DUET geometry"):
            eng.forward(b["query"], b["query_idf"], torch.cat([b["posdoc"], b["posdoc"][:, :1]], dim=1), m._params())
        with pytest.raises(ValueError, match="unsupported DUET geometry"):
            eng.forward(torch.cat([b["query"], b["query"][:, :1]], dim=1), torch.cat([b["query_idf"], b["query_idf"][:, :1]], dim=1), b["posdoc"],
                        m._params())
        assert torch.isfinite(r.test(b)).all()


def test_score_in_training_mode_runs_the_restatement_with_gradients():
    c = duet_case.load("duet_grad")
    r, m = _plugin("duet_grad")
    m.train()
    b = _batch(c["query"], c["posdoc"], c["query_idf"])
    b["negdoc"] = torch.from_numpy(c["negdoc"]).to(DEV)
    pos, neg = r.score(b)
    assert pos.requires_grad and neg.requires_grad and pos.shape == neg.shape == (c["query"].shape[0],)
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().cpu().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"]).to(DEV)).sum().backward()
    for k in ("lm.conv.0.weight", "lm.ffw.0.weight", "dm.q_conv.0.weight", "dm.d_conv1.0.weight", "dm.d_conv2.0.weight", "dm.ffw_1.0.weight"):
        g, want = dict(m.named_parameters())[k].grad.cpu().numpy(), c["grad." + k]
        assert np.abs(g - want).max() <= 1e-4 * np.abs(want).max(), k
