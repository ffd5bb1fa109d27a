"""POSITDRMM (reranker `POSITDRMM`) on the MI355X: capamd_posit_forward (csrc/posit.hip) against the float64 restatement on the same
inputs and against the reference's fixtures (tests/golden/posit_*.npz), its invariances (micro-batch size, chunk length, tile mates), the
match statistics, and the refusals.

The tolerance is not a constant: per quantity max(4 e_ref, 16 fp32 ulp of its largest magnitude in the case), with e_ref the reference's
own fp32 error on that case (posit_case.yardstick).  Every figure is printed before it is asserted.

Which case reaches which instantiation of the launcher (rec_kernel<NB>, NB = padded width / 64; the sequence tile is 16 everywhere):
NB = 1: every fixture of dim 24; NB = 5: posit_dim300 (17 pairs: a full tile and a ragged second one); NB = 2, 3, 4: WIDTHS below.  The
projection GEMM's column tiles: 4 NB % 3 == 0 only at NB = 3 (gemm_kernel<2, 3>), gemm_kernel<2, 2> at the others.  More than one chunk
of steps per layer: test_chunked_steps_give_the_same_bits (two chunks at NB = 1).

Every case here has Q <= 4, pad columns in its width and at most one of a row's five largest per lane of the pooling wave.  The rest of
the geometry - Q = 5 .. 16, document lengths around 64 / 128 / 320 and at 8192, widths with Dp == D at every NB, six candidates in one
lane, batches around the sequence tile, three chunks at NB = 3 and 5 and a chunked query side - is in tests/test_gpu_posit_geometry.py,
whose docstring says which point reaches which instantiation."""
import numpy as np
import pytest
import torch

from capreolus_amd.reranker import POSITDRMM
from capreolus_amd.reranker.POSITDRMM import exact_match_stats
from tests import posit_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _plugin(name):
    r, m = posit_case.build(name, POSITDRMM)
    m.to(DEV).eval()
    return r, m


def _dev(c, *keys):
    return [torch.from_numpy(c[k]).to(DEV) for k in keys]


def _check(tag, got, f64, e_ref):
    err, b = float(np.abs(got - f64).max()), posit_case.bound(e_ref, np.abs(f64).max())
    print(f"\n{tag}: e_ref {e_ref:.3g} bound {b:.3g} kernel-vs-f64 {err:.3g} scale {np.abs(f64).max():.3g}")
    assert np.all(np.isfinite(got)), tag
    return err <= b, (tag, err, b)


@pytest.mark.parametrize("name", posit_case.SCORE_CASES)
def test_scores_features_and_contexts_against_float64_and_the_reference(name):
    c = posit_case.load(name)
    f64, e_ref = posit_case.yardstick(name, POSITDRMM)
    r, m = _plugin(name)
    q, idf, d, ex = _dev(c, "query", "query_idf", "posdoc", "extras")
    with torch.no_grad():
        score, det = m.forward_engine(d, q, idf, extras=ex, details=True)
        assert torch.equal(m.test_forward(q, idf, d, ex), score) and score.dtype == torch.float32
    pairs = posit_case.context_pairs(name)
    got = {"score": score.cpu().numpy(), "features": det["features"].cpu().numpy(),
           "query_context": det["query_context"].cpu().numpy()[pairs], "doc_context": det["doc_context"].cpu().numpy()[pairs]}
    # (posit_long records no context tensors, so there is no e_ref for them: they are held through the features there)
    verdicts = [_check(f"{name} {k}", got[k], f64[k], e_ref[k]) for k in ("query_context", "doc_context", "features", "score") if k in e_ref]
    err_fix, b = np.abs(got["score"] - c["score"]).max(), posit_case.bound(e_ref["score"], np.abs(f64["score"]).max())
    print(f"\n{name}: kernel-vs-fixture scores {err_fix:.3g}")
    for ok, why in verdicts:
        assert ok, why
    assert err_fix <= b, (err_fix, b)
    # the exact-match features hold only counts: the reference's bits
    assert np.array_equal(got["features"][:, :, 4:], c["features"][:, :, 4:])


@pytest.mark.parametrize("name", list(posit_case.SCORE_CASES) + ["posit_grad"])
def test_match_statistics_on_the_device_equal_the_host_and_the_reference(name):
    c = posit_case.load(name)
    r, m = _plugin(name)
    q, idf, d, ex, bm25 = _dev(c, "query", "query_idf", "posdoc", "extras", "bm25")
    B = q.shape[0]
    r.searcher_scores = {"q": {f"d{i}": float(v) for i, v in enumerate(c["bm25"])}}
    batch = {"query": q, "query_idf": idf, "posdoc": d, "qid": ["q"] * B, "posdocid": [f"d{i}" for i in range(B)]}
    with torch.no_grad():
        score, det = m.forward_engine(d, q, idf, bm25=bm25, details=True)
        from_extras = m.forward_engine(d, q, idf, extras=ex)
        test = r.test(batch)
    host = torch.cat(exact_match_stats(torch.from_numpy(c["query_idf"]), torch.from_numpy(c["query"]), torch.from_numpy(c["posdoc"]), 0), dim=1)
    on_device = torch.cat(r.get_exact_match_stats(idf, q, d), dim=1)
    assert on_device.is_cuda and torch.equal(on_device.cpu(), host)
    assert np.array_equal(det["stats"].cpu().numpy(), c["stats"]) and torch.equal(det["stats"].cpu(), host)
    assert torch.equal(score, from_extras) and torch.equal(test, score)


def test_scores_do_not_depend_on_microbatch_size_or_tile_mates():
    c = posit_case.load("posit_dim300")
    r, m = _plugin("posit_dim300")
    q, idf, d, ex = _dev(c, "query", "query_idf", "posdoc", "extras")
    with torch.no_grad():
        whole, det = m.forward_engine(d, q, idf, extras=ex, details=True)
        for nb in (1, 16):
            m._engine.docs_per_microbatch = nb
            s, dt = m.forward_engine(d, q, idf, extras=ex, details=True)
            assert torch.equal(s, whole), nb
            for k in det:
                assert torch.equal(dt[k], det[k]), (nb, k)
        m._engine.docs_per_microbatch = None
        # other tile mates, another place in the tile
        perm = torch.arange(16, -1, -1, device=DEV)
        assert torch.equal(m.forward_engine(d[perm], q[perm], idf[perm], extras=ex[perm]), whole[perm])
        assert torch.equal(m.forward_engine(d[5:8], q[5:8], idf[5:8], extras=ex[5:8]), whole[5:8])


def test_chunked_steps_give_the_same_bits():
    """400 pairs of 800 steps at the padded width 64 need more than the 512 MiB of projections a chunk may take: the layers run in two
    chunks of steps (655 + 145), with c handed over through the state buffer and h read back from the output"""
    c = posit_case.load("posit_long")
    r, m = _plugin("posit_long")
    q, idf, d, ex = _dev(c, "query", "query_idf", "posdoc", "extras")
    idx = torch.arange(400, device=DEV) % q.shape[0]
    with torch.no_grad():
        five, det5 = m.forward_engine(d, q, idf, extras=ex, details=True)
        m._engine.docs_per_microbatch = 400
        many, det = m.forward_engine(d[idx], q[idx], idf[idx], extras=ex[idx], details=True)
    assert torch.equal(many, five[idx])
    assert torch.equal(det["features"], det5["features"][idx]) and torch.equal(det["doc_context"][395:], det5["doc_context"])


WIDTHS = ((100, 2), (150, 3), (200, 4))


@pytest.mark.parametrize("D,NB", WIDTHS)
def test_every_padded_width_against_float64(D, NB):
    """the widths between the fixtures' (no recorded reference: e_ref is the fp32 restatement's error, which reproduces the reference bit
    for bit on every fixture, tests/test_posit_cpu.py); 3 pairs of 2 x 6 terms"""
    from types import SimpleNamespace

    assert (D + 63) // 64 == NB
    rs = np.random.RandomState(D)
    ex = SimpleNamespace(embeddings=posit_case.make_embeddings(rs, d=D), pad=0, config={})
    w = posit_case.make_weights(rs, D)
    q, d = rs.randint(1, posit_case.V, size=(3, 2)).astype(np.int64), rs.randint(0, posit_case.V, size=(3, 6)).astype(np.int64)
    d[:, :2], q[1, 1], d[1, 4:] = q, 0, 0
    idf, extras = (rs.rand(3, 2) * 3).astype(np.float32), rs.rand(3, 4).astype(np.float32)
    host = posit_case.build_from(ex, w, POSITDRMM)[1].eval()
    t = [torch.from_numpy(a) for a in (d, q, idf, extras)]
    with torch.no_grad():
        s64, d64 = host._forward_aten(*t, dtype=torch.float64, return_details=True)
        s32, d32 = host._forward_aten(*t, return_details=True)
        m = posit_case.build_from(ex, w, POSITDRMM)[1].to(DEV).eval()
        score, det = m.forward_engine(*(a.to(DEV) for a in t[:3]), extras=t[3].to(DEV), details=True)
    verdicts = [_check(f"dim {D} score", score.cpu().numpy(), s64.numpy(), float((s32 - s64).abs().max()))]
    for k in ("features", "query_context", "doc_context"):
        verdicts.append(_check(f"dim {D} {k}", det[k].cpu().numpy(), d64[k].numpy(), float((d32[k] - d64[k]).abs().max())))
    for ok, why in verdicts:
        assert ok, why


def test_forward_of_a_training_pair_in_eval_mode():
    c = posit_case.load("posit_grad")
    r, m = _plugin("posit_grad")
    host = posit_case.build("posit_grad", POSITDRMM)[1].eval()
    t = {k: torch.from_numpy(c[k]) for k in ("query", "query_idf", "posdoc", "negdoc", "extras", "neg_extras")}
    with torch.no_grad():
        s64 = torch.cat([host._forward_aten(t[dk], t["query"], t["query_idf"], t[ek], dtype=torch.float64)
                         for dk, ek in (("posdoc", "extras"), ("negdoc", "neg_extras"))]).numpy()
    g = {k: v.to(DEV) for k, v in t.items()}
    pos, neg = m(g["query"], g["query_idf"], g["posdoc"], g["negdoc"], g["extras"], g["neg_extras"])      # eval mode, grad enabled: the kernels
    got = torch.cat([pos, neg]).cpu().numpy()
    ok, why = _check("posit_grad score", got, s64, float(np.abs(c["score"] - s64).max()))
    assert ok, why


def test_status_bits_and_refusals_raise():
    c = posit_case.load("posit_small")
    r, m = _plugin("posit_small")
    q, idf, d, ex = _dev(c, "query", "query_idf", "posdoc", "extras")
    with torch.no_grad():
        good = m.forward_engine(d, q, idf, extras=ex)
        bad = d.clone()
        bad[1, 0] = posit_case.V
        with pytest.raises(ValueError, match="document term id"):
            m.forward_engine(bad, q, idf, extras=ex)
        badq = q.clone()
        badq[0, 0] = -3
        with pytest.raises(ValueError, match="query term id"):
            m.forward_engine(d, badq, idf, extras=ex)
        short = d.clone()
        short[2, 1:] = 0
        with pytest.raises(ValueError, match="fewer than 2"):
            m.forward_engine(short, q, idf, extras=ex)
        with pytest.raises(ValueError, match="at least 5"):
            m.forward_engine(d[:, :4], q, idf, extras=ex)
        with pytest.raises(ValueError, match="geometry"):
            m.forward_engine(d, q.repeat(1, 6), idf.repeat(1, 6), extras=ex)        # Q = 18
        with pytest.raises(ValueError, match="either"):
            m.forward_engine(d, q, idf)
        assert torch.equal(m.forward_engine(d, q, idf, extras=ex), good)            # the status word is clean again
