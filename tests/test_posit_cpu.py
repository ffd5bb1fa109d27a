"""POSITDRMM (reranker `POSITDRMM`) on the host: the plugin's parameter surface against the reference's (fixtures made by
tests/golden/make_golden_posit.py from the reference POSITDRMM_class), checkpoints, refusals, the C ABI's limits, the match statistics
against the reference's loops, and the restatement against the reference's outputs in fp32 and in float64 (e_ref, the yardstick of the
device tests: max(4 e_ref, 16 ulp) per quantity)."""
import ctypes

import numpy as np
import pytest
import torch

from capreolus_amd import _lib, reranker
from capreolus_amd.reranker import POSITDRMM, POSITDRMM_basic, POSITDRMM_class
from capreolus_amd.reranker.POSITDRMM import exact_match_stats
from tests import posit_case

STATE_KEYS = ["posit1.embedding.weight"] + [f"posit1.encoding_layer.{k}_l{n}{rev}" for n in (0, 1) for rev in ("", "_reverse")
                                            for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + [
    "posit1.Q1.weight", "posit1.Q1.bias", "posit1.Wg.weight", "posit1.Wg.bias"]


def _model(name):
    return posit_case.build(name, POSITDRMM)


def test_plugin_surface():
    assert POSITDRMM.module_name == "POSITDRMM" and POSITDRMM.config_spec == {}
    assert "POSITDRMM" not in reranker.registry
    assert reranker.POSITDRMM is POSITDRMM and reranker.POSITDRMM_class is POSITDRMM_class and reranker.POSITDRMM_basic is POSITDRMM_basic
    with pytest.raises(ValueError):
        POSITDRMM({"nosuchoption": 1}, posit_case.extractor("posit_small"))
    _, m = _model("posit_small")
    lstm = m.posit1.encoding_layer
    assert isinstance(lstm, torch.nn.LSTM) and (lstm.input_size, lstm.hidden_size, lstm.num_layers, lstm.bidirectional, lstm.dropout) == (
        posit_case.D, posit_case.D, 2, True, 0.3)


@pytest.mark.parametrize("name", list(posit_case.CASES))
def test_state_dict_is_the_references_and_round_trips(name):
    c = posit_case.load(name)
    r, m = _model(name)
    sd = m.state_dict()
    assert sorted(sd) == list(c["state_keys"]) == sorted(STATE_KEYS)
    for k, shape in zip(c["state_keys"], c["state_shapes"]):
        assert list(sd[k].shape) == [int(x) for x in shape[: sd[k].dim()]], k
    r2, m2 = posit_case.build_from(posit_case.extractor(name), posit_case.make_weights(np.random.RandomState(1), posit_case.dim(name)), POSITDRMM)
    m2.load_state_dict(sd)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert not m.posit1.embedding.weight.requires_grad


@pytest.mark.parametrize("name", list(posit_case.CASES))
def test_fixture_ids_are_what_posit_case_draws(name):
    c = posit_case.load(name)
    ins = posit_case.inputs(name)
    for k, v in zip(("query", "posdoc", "query_idf", "bm25", "negdoc", "neg_bm25"), ins):
        assert np.array_equal(c[k], v), k
    posit_case.check_ids(ins[0], ins[1])
    emb = posit_case.embeddings(name)
    assert not emb[0].any() and 0.5e-7 < np.linalg.norm(emb[posit_case.TINY_TOKEN]) < 2e-7


def _restated(name, dtype):
    c = posit_case.load(name)
    m = _model(name)[1].eval()
    with torch.no_grad():
        score, det = m._forward_aten(torch.from_numpy(c["posdoc"]), torch.from_numpy(c["query"]), torch.from_numpy(c["query_idf"]),
                                     torch.from_numpy(c["extras"]), dtype=dtype, return_details=True)
    pairs = posit_case.context_pairs(name)
    return {"score": score.numpy(), "features": det["features"].numpy(), "query_context": det["query_context"].numpy()[pairs],
            "doc_context": det["doc_context"].numpy()[pairs]}


@pytest.mark.parametrize("name", posit_case.SCORE_CASES)
def test_restatement_in_fp32_reproduces_the_reference(name):
    got, ref = _restated(name, torch.float32), posit_case.reference_outputs(name)
    f64, e_ref = posit_case.yardstick(name, POSITDRMM)
    assert set(ref) == {"score", "features"} | ({"query_context", "doc_context"} if name in posit_case.CONTEXT_CASES else set())
    for k in ref:
        assert got[k].dtype == np.float32 and got[k].shape == ref[k].shape and np.all(np.isfinite(got[k])), k
        err, b = np.abs(got[k] - ref[k]).max(), posit_case.bound(e_ref[k], np.abs(f64[k]).max())
        print(f"\n{name} {k}: restatement-vs-reference {err:.3g} bound {b:.3g}")
        assert err <= b, (k, err, b)


@pytest.mark.parametrize("name", posit_case.SCORE_CASES)
def test_float64_restatement_gives_the_references_own_error(name):
    """e_ref per quantity (DESIGN §3.9 tabulates what this prints): small against the quantity's scale, and not zero"""
    f64, e_ref = posit_case.yardstick(name, POSITDRMM)
    for k, e in e_ref.items():
        scale = np.abs(f64[k]).max()
        print(f"\n{name} {k}: e_ref {e:.3g} scale {scale:.3g} bound {posit_case.bound(e, scale):.3g}")
        assert f64[k].dtype == np.float64
        assert 0 < e <= 1e-4 * scale, (k, e, scale)


def test_restatement_gradients_match_the_reference():
    c = posit_case.load("posit_grad")
    r, m = _model("posit_grad")
    m.eval()
    t = {k: torch.from_numpy(c[k]) for k in ("query", "query_idf", "posdoc", "negdoc", "extras", "neg_extras")}
    with torch.enable_grad():
        score = torch.cat([m._forward_aten(t["posdoc"], t["query"], t["query_idf"], t["extras"]),
                           m._forward_aten(t["negdoc"], t["query"], t["query_idf"], t["neg_extras"])])
        (score * torch.from_numpy(c["loss_coef"])).sum().backward()
    np.testing.assert_allclose(score.detach().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    names = [k[len("grad."):] for k in c if k.startswith("grad.")]
    assert set(names) == {k for k, p in m.named_parameters() if p.requires_grad}
    params = dict(m.named_parameters())
    for k in names:
        want, got = c["grad." + k], params[k].grad.numpy()
        assert np.abs(got - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6), (k, np.abs(got - want).max(), np.abs(want).max())


def test_training_mode_runs_the_restatement_under_autograd_with_dropout():
    c = posit_case.load("posit_grad")
    r, m = _model("posit_grad")
    r.searcher_scores = {"q": {f"p{i}": float(v) for i, v in enumerate(c["bm25"])} | {f"n{i}": float(v) for i, v in enumerate(c["neg_bm25"])}}
    B = c["query"].shape[0]
    d = {k: torch.from_numpy(c[k]) for k in ("query", "query_idf", "posdoc", "negdoc")}
    d.update(qid=["q"] * B, posdocid=[f"p{i}" for i in range(B)], negdocid=[f"n{i}" for i in range(B)])
    m.train()
    torch.manual_seed(3)
    pos, neg = r.score(d)
    assert pos.requires_grad and pos.shape == (B,) and neg.shape == (B,)
    torch.manual_seed(4)
    pos2, _ = r.score(d)
    assert not torch.equal(pos, pos2)          # the dropouts are live
    (pos - neg).sum().backward()
    assert all(p.grad is not None for k, p in m.named_parameters() if p.requires_grad)


@pytest.mark.parametrize("name", list(posit_case.CASES))
def test_vectorised_match_statistics_equal_the_references_loops(name):
    c = posit_case.load(name)
    for doc_key, stats_key in (("posdoc", "stats"), ("negdoc", "neg_stats")):
        if doc_key not in c:
            continue
        got = torch.cat(exact_match_stats(torch.from_numpy(c["query_idf"]), torch.from_numpy(c["query"]), torch.from_numpy(c[doc_key]), 0), dim=1).numpy()
        assert got.dtype == np.float32 and got.shape == c[stats_key].shape
        assert np.array_equal(got, c[stats_key]), (got, c[stats_key])                  # the reference plugin's own output, bit for bit
        assert np.array_equal(got, posit_case.loop_stats(c["query_idf"], c["query"], c[doc_key]))
    if name == "posit_ties":
        q, d = c["query"], c["posdoc"]
        cnt = [(d[b] == q[b, 0]).sum() for b in range(3)]
        assert cnt[0] < 5 and cnt[1] == 5 and cnt[2] > 5
        assert c["stats"][4, 2] == np.float32(2 / 3)        # the query bigram, once plainly and once across a removed pad, of 3 bigrams
        assert c["stats"][3].tolist() == [0.0, 0.0, 0.0]    # an all-pad query matches nothing in a cleaned document


def test_match_statistics_on_random_ids_with_pads_anywhere():
    rs = np.random.RandomState(5)
    q = rs.randint(0, 6, size=(40, 5)).astype(np.int64)
    d = rs.randint(0, 6, size=(40, 23)).astype(np.int64)
    d[:, :2] = rs.randint(1, 6, size=(40, 2))
    idf = (rs.rand(40, 5) * 3).astype(np.float32)
    got = torch.cat(exact_match_stats(torch.from_numpy(idf), torch.from_numpy(q), torch.from_numpy(d), 0), dim=1).numpy()
    assert np.array_equal(got, posit_case.loop_stats(idf, q, d))


# ---- the preconditions of the geometry sweep (tests/test_gpu_posit_geometry.py) -----------------------------------------------------------
SWEEP_POINTS = ([(24, Q, 40, 5) for Q in (1, 2, 4, 5, 6, 7, 8, 9, 12, 13, 15, 16)] + [(300, 16, 40, 17), (24, 5, 5, 3), (24, 5, 321, 3), (24, 4, 8192, 2),
                (1, 5, 17, 3), (320, 5, 17, 3), (64, 5, 17, 33)] + [p[:3] + (posit_case.CHUNK_BASE_PAIRS,) for p, _, _ in posit_case.CHUNK_POINTS.values()])


@pytest.mark.parametrize("D,Q,L,B", SWEEP_POINTS)
def test_sweep_case_draws_the_id_patterns_it_promises(D, Q, L, B):
    c = posit_case.sweep_case(D, Q, L, B)
    q, d = c["query"], c["posdoc"]
    posit_case.check_sweep_ids(q, d)
    assert posit_case.sweep_case(D, Q, L, B) is c                                     # made once
    assert q.shape == (B, Q) and d.shape == (B, L) and q.dtype == d.dtype == np.int64 and q.max() < posit_case.V and d.max() < posit_case.V
    assert c["query_idf"].shape == (B, Q) and c["extras"].shape == (B, 4) and np.array_equal(c["bm25"], c["extras"][:, 3])
    emb = c["ex"].embeddings
    assert emb.shape == (posit_case.V, D) and not emb[0].any() and 0.5e-7 < np.linalg.norm(emb[posit_case.TINY_TOKEN]) < 2e-7
    if Q > 4:
        # the pad query term and the repeated one sit in the last group of four, which a later pass of cos_pass handles
        assert (np.nonzero(q[1 % B] == 0)[0] >= 4 * ((Q - 1) // 4)).all()
        assert q[2 % B, 4 * ((Q - 1) // 4)] == q[2 % B, 0]
    stats = posit_case.loop_stats(c["query_idf"], q, d)
    host = torch.cat(exact_match_stats(torch.from_numpy(c["query_idf"]), torch.from_numpy(q), torch.from_numpy(d), 0), dim=1).numpy()
    assert np.array_equal(stats, host)


def test_sweep_yardstick_is_the_restatements_own_error():
    c = posit_case.sweep_case(24, 9, 40, 5)
    f64, e_ref = posit_case.sweep_yardstick(c, POSITDRMM)
    assert posit_case.sweep_yardstick(c, POSITDRMM)[0] is f64 and set(f64) == set(e_ref) == set(posit_case.QUANTITIES)
    for k in posit_case.QUANTITIES:
        scale = np.abs(f64[k]).max()
        print(f"\n(24, 9, 40, 5) {k}: e_ref {e_ref[k]:.3g} scale {scale:.3g} bound {posit_case.bound(e_ref[k], scale):.3g}")
        assert f64[k].dtype == np.float64 and 0 < e_ref[k] <= 1e-4 * scale, (k, e_ref[k], scale)
    assert f64["features"].shape == (5, 9, 6) and f64["doc_context"].shape == (5, 40, 48)


@pytest.mark.parametrize("variant", posit_case.LANE_VARIANTS)
def test_lane_variants_put_six_candidates_into_one_lane(variant):
    """the preconditions of test_top5_of_one_lane, on float64 alone (posit_case.check_lane)"""
    c = posit_case.lane_case(variant)
    f64, e_ref = posit_case.sweep_yardstick(c, POSITDRMM)
    b = posit_case.bound(e_ref["features"], np.abs(f64["features"]).max())
    posit_case.check_lane(c, b)
    row, top = posit_case.lane_row(c)
    # the float64 restatement pools that row: its max and the mean of its five largest
    assert abs(f64["features"][0, 0, 0] - row[top[0]]) < 1e-12 and abs(f64["features"][0, 0, 1] - row[top[:5]].sum() / 5) < 1e-12
    assert ((c["posdoc"] != 0).sum(1) >= 2).all() and c["posdoc"].shape == (3, 400)
    if variant == "ties":
        assert f64["features"][0, 0, 5] == 1.0 and (c["posdoc"][0] == c["query"][0, 0]).sum() == 6
    # a lane that kept four of its six would give (for the first three variants) the 7th largest in place of the 5th
    if variant != "decoy":
        assert (row[top[4]] - row[top[6]]) / 5 > 1000 * b


def test_chunk_arithmetic_of_the_chunk_points():
    """the chunk lengths the GPU tests claim follow from posit.hip's chunk_steps, and the library's workspace is the one carve lays out
    for that T - one step more or less per chunk is another size (no device access)"""
    lib = _lib.load()
    for name, ((D, Q, L, n), (T, q_chunks, d_chunks), NB) in posit_case.CHUNK_POINTS.items():
        assert posit_case.chunk_steps(n, D, Q, L) == T and (D + 63) // 64 == NB, name
        assert posit_case.chunks(Q, T) == q_chunks and posit_case.chunks(L, T) == d_chunks, name
        assert sum(q_chunks) == Q and sum(d_chunks) == L and max(len(q_chunks), len(d_chunks)) >= 2
        m = _lib.PositModel()
        m.vocab, m.pad, m.dim = posit_case.V, 0, D
        got = lib.capamd_posit_workspace_bytes(ctypes.byref(m), n, Q, L)
        assert got == posit_case.workspace_bytes(n, D, Q, L, T), (name, got)
        assert got not in (posit_case.workspace_bytes(n, D, Q, L, T - 1), posit_case.workspace_bytes(n, D, Q, L, T + 1))
        # the five base pairs run in one chunk per side
        T0 = posit_case.chunk_steps(posit_case.CHUNK_BASE_PAIRS, D, Q, L)
        assert posit_case.chunks(Q, T0) == [Q] and posit_case.chunks(L, T0) == [L]
    assert posit_case.CHUNK_POINTS["three_chunks_gemm_tile_3"][1:] == ((87, [4], [87, 87, 26]), 3)       # 4 NB % 3 == 0: gemm_kernel<2, 3>
    assert posit_case.CHUNK_POINTS["three_chunks_widest"][1:] == ((52, [4], [52, 52, 16]), 5)
    assert posit_case.CHUNK_POINTS["chunked_query_one_step"][1][1] == [15, 1]
    # the fixture test of two chunks (test_chunked_steps_give_the_same_bits): 655 + 145
    assert posit_case.chunks(800, posit_case.chunk_steps(400, 24, 4, 800)) == [655, 145]


def test_matching_case_tells_a_fused_idf_sum_from_the_references():
    q, d, idf, bm25 = posit_case.matching_case()
    loops = posit_case.loop_stats(idf, q, d)
    host = torch.cat(exact_match_stats(torch.from_numpy(idf), torch.from_numpy(q), torch.from_numpy(d), 0), dim=1).numpy()
    assert np.array_equal(host, loops) and (loops > 0).all() and ((d != 0).sum(1) >= 2).all()
    fused = posit_case.fused_idf_stat(idf, q, d)
    print(f"\npairs whose idf statistic a fused multiply-add rounds differently: {int((fused != loops[:, 1]).sum())} of {len(fused)}")
    assert (fused != loops[:, 1]).sum() >= 3 and np.abs(fused - loops[:, 1]).max() <= 2 * np.spacing(loops[:, 1].max())
    # ... and the sweep point that found it: pair 2 of (24, 7, 40, 5), whose query repeats a term the document holds seven times
    c = posit_case.sweep_case(24, 7, 40, 5)
    assert posit_case.fused_idf_stat(c["query_idf"], c["query"], c["posdoc"])[2] != posit_case.loop_stats(c["query_idf"], c["query"], c["posdoc"])[2, 1]


def test_refusals():
    c = posit_case.load("posit_small")
    r, m = _model("posit_small")
    m.eval()
    q, idf, ex = torch.from_numpy(c["query"]), torch.from_numpy(c["query_idf"]), torch.from_numpy(c["extras"])
    d = torch.from_numpy(c["posdoc"])
    with torch.no_grad():
        with pytest.raises(ValueError, match="at least 5"):
            m._forward_aten(d[:, :4], q, idf, ex)
        with pytest.raises(ValueError, match="at least 5"):
            m.forward_engine(d[:, :4], q, idf, extras=ex)
    short = d.clone()
    short[2, 1:] = 0
    with pytest.raises(ValueError, match="fewer than 2"):
        r.get_exact_match_stats(idf, q, short)
    wide = posit_case.extractor("posit_small")
    wide.embeddings = np.zeros((8, 321), dtype=np.float32)
    with pytest.raises(ValueError, match="dim"):
        POSITDRMM({}, wide).build_model()


def test_scoring_without_a_device_is_an_error_not_a_fallback():
    c = posit_case.load("posit_five")
    r, m = _model("posit_five")
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        m.test_forward(torch.from_numpy(c["query"]), torch.from_numpy(c["query_idf"]), torch.from_numpy(c["posdoc"]), torch.from_numpy(c["extras"]))


def test_c_abi_signature_version_and_limits():
    """capamd_posit_workspace_bytes / capamd_posit_forward answer -1 / CAPAMD_ERR_ARG to what the kernels do not take (no device access)"""
    lib = _lib.load()
    assert _lib.VERSION == 405 and lib.capamd_version() == 405 and _lib.STATUS_SHORT_DOC == 64
    assert "capamd_posit_forward" in _lib.SIGNATURES and "capamd_posit_workspace_bytes" in _lib.SIGNATURES
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "capreolus_amd.h")).read()
    assert "#define CAPAMD_VERSION 405" in header and "capamd_posit_model" in header
    P = ctypes.c_void_p(4096)

    def model(**kw):
        m = _lib.PositModel()
        m.emb = m.q1_w = m.q1_b = m.wg_w = m.wg_b = 4096
        for n in range(2):
            m.w_ih[n] = m.w_hh[n] = m.bias[n] = 4096
        m.vocab, m.pad, m.dim = 64, 0, 300
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    def fwd(m, B=8, Q=4, L=800, nb=4, ws=P, ws_bytes=1 << 40, extras=P, bm25=None):
        return lib.capamd_posit_forward(P, P, P, extras, bm25, B, Q, L, ctypes.byref(m), nb, ws, ws_bytes, P, None, None, None, None, P, None)

    assert lib.capamd_posit_workspace_bytes(ctypes.byref(model()), 4, 4, 800) > 0
    assert lib.capamd_posit_workspace_bytes(ctypes.byref(model(dim=320)), 1, 16, 8192) > 0
    # about 5 MB per pair of 4 x 800 at dim 300, next to the 512 MiB of input projections
    per_pair = (lib.capamd_posit_workspace_bytes(ctypes.byref(model()), 101, 4, 800) - lib.capamd_posit_workspace_bytes(ctypes.byref(model()), 1, 4, 800)) / 100
    assert 4e6 < per_pair < 12e6, per_pair
    for mkw, skw in (({"dim": 321}, {}), ({"dim": 0}, {}), ({"vocab": 0}, {}), ({}, {"Q": 17}), ({}, {"Q": 0}), ({}, {"L": 4}), ({}, {"L": 8193}),
                     ({}, {"nb": 0})):
        m = model(**mkw)
        Q, L, nb = skw.get("Q", 4), skw.get("L", 800), skw.get("nb", 4)
        assert lib.capamd_posit_workspace_bytes(ctypes.byref(m), nb, Q, L) == -1, (mkw, skw)
        assert fwd(m, Q=Q, L=L, nb=nb) == _lib.ERR_ARG, (mkw, skw)
    assert lib.capamd_posit_workspace_bytes(None, 4, 4, 800) == -1
    assert fwd(model(), extras=None, bm25=None) == _lib.ERR_ARG          # one of the two must be there
    assert fwd(model(), B=-1) == _lib.ERR_ARG
    for n in ("emb", "q1_w", "q1_b", "wg_w", "wg_b"):
        assert fwd(model(**{n: None})) == _lib.ERR_ARG, n
    m = model()
    m.w_hh[1] = None
    assert fwd(m) == _lib.ERR_ARG
    m = model()
    m.w_ih[0] = 4100
    assert fwd(m) == _lib.ERR_ALIGN
    # an empty call is fine; a short or misaligned workspace is named as such, before anything is launched
    assert fwd(model(), B=0) == _lib.OK
    assert fwd(model(), ws_bytes=1000) == _lib.ERR_WORKSPACE
    assert fwd(model(), ws=ctypes.c_void_p(4096 + 16)) == _lib.ERR_ALIGN
