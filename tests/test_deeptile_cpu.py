"""DeepTileBar (reranker `DeepTileBar`) on the host: the plugin's configuration and parameter surface against the reference's (fixtures
made by tests/golden/make_golden_deeptile.py from the reference's DeepTileExtractor and DeepTileBar_class), checkpoints, refusals, the C
ABI, the host side of the colouring, and the restatements against the reference's tiles, scores, W1 input and gradients.

The tolerance is the project's rule, not a constant: per output e_ref = max |fixture - float64 restatement| is the reference's own fp32
error, and what is tested gets max(4 e_ref, 16 fp32 ulp of the output's scale).  Integer-valued channels are exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

from capreolus_amd import deeptiles, reranker
from capreolus_amd.reranker import DeepTileBar, DeepTileBar_class
from tests import deeptile_case


def _model(name):
    return deeptile_case.build(name, DeepTileBar)


def _bound(e_ref, scale):
    return max(4.0 * e_ref, 16.0 * float(np.spacing(np.float32(scale))))


def test_config_options_and_defaults():
    assert DeepTileBar.module_name == "DeepTileBar"
    assert DeepTileBar.config_spec == {"passagelen": 30, "numberfilter": 3, "lstmhiddendim": 3, "linearhiddendim1": 32, "linearhiddendim2": 16}
    assert not DeepTileBar.supports_resident and not DeepTileBar.supports_lists
    assert "DeepTileBar" not in reranker.registry and reranker.DeepTileBar is DeepTileBar and reranker.DeepTileBar_class is DeepTileBar_class
    with pytest.raises(ValueError):
        DeepTileBar({"nosuchoption": 1}, deeptile_case.extractor("deeptile_default"))


@pytest.mark.parametrize("name", list(deeptile_case.CASES))
def test_state_dict_names_and_shapes_match_the_reference(name):
    c = deeptile_case.load(name)
    _, m = _model(name)
    sd = m.state_dict()
    assert sorted(sd) == [str(k) for k in c["state_keys"]]
    for k, shape in zip(c["state_keys"], c["state_shapes"]):
        assert list(sd[str(k)].shape) == [int(x) for x in shape if x], k
    assert len(sd) == 20 + 40 + 6


@pytest.mark.parametrize("name", list(deeptile_case.CASES))
def test_encode_segments_reproduces_the_fixture_ids_and_offsets(name):
    c = deeptile_case.load(name)
    case = deeptile_case.CASES[name]
    deeptile_case.check_text(name)
    stoi = deeptile_case.vocabulary()
    for b, segs in enumerate(c["segments"]):
        row, off = deeptiles.encode_segments([str(s) for s in segs], stoi, deeptile_case.PAD_TOK, case["P"], case["L"])
        np.testing.assert_array_equal(off, c["posdoc_segments"][b])
        np.testing.assert_array_equal(row[:off[-1]], c["posdoc"][b, :off[-1]])
        assert row.dtype == np.int64 and off.dtype == np.int32 and row.shape == (case["L"],) and not row[off[-1]:].any()
    q = np.array([[stoi.get(str(t), 0) for t in row] for row in c["query_toks"]])
    np.testing.assert_array_equal(q, c["query"])


def test_encode_segments_string_handling():
    stoi = {"<pad>": 0, "a": 1, "b": 2}
    row, off = deeptiles.encode_segments(["a b a", "<pad>", "", "a <pad> zz", "b", "never"], stoi, "<pad>", 5)
    assert off.tolist() == [0, 3, 3, 4, 7, 8] and row.tolist() == [1, 2, 1, 0, 1, -1, 0, 2]
    assert deeptiles.encode_segments(["a  b"], stoi, "<pad>", 1)[0].tolist() == [1, 0, 2]       # split(" "): an empty token between two blanks
    with pytest.raises(ValueError):
        deeptiles.encode_segments(["a b a"], stoi, "<pad>", 1, L=2)
    with pytest.raises(ValueError):
        deeptiles.encode_segments(["a"], stoi, "<pad>", 2)


@pytest.mark.parametrize("name", list(deeptile_case.CASES))
def test_numpy_colouring_matches_the_reference_tiles(name):
    c = deeptile_case.load(name)
    C, D = deeptile_case.CASES[name]["C"], deeptile_case.CASES[name]["D"]
    emb = deeptile_case.embeddings(name)
    args = (c["query"], c["posdoc"], c["posdoc_segments"], c["query_idf"], emb, C)
    t64, t32 = deeptiles.color_numpy(*args), deeptiles.color_numpy(*args, dtype=np.float32)
    want = c["tiles"]
    assert t64.shape == want.shape == (c["query"].shape[0], c["query"].shape[1], c["posdoc_segments"].shape[1] - 1, C)
    np.testing.assert_array_equal(t64[..., :-1].astype(np.float32), want[..., :-1])          # tf and idf: exact
    np.testing.assert_array_equal(t32[..., :-1], want[..., :-1])
    e_ref = float(np.abs(want[..., -1] - t64[..., -1]).max())
    err = float(np.abs(t32[..., -1] - t64[..., -1]).max())
    # sim = exp(-d2 / 2): its relative error is the absolute error of d2 / 2, and d2 is D squares of fp32 differences summed, a root and a
    # square: at most (D + 8) eps of d2 - the reference cannot be further from float64 than that at the smallest live sim
    d2half = -np.log(want[..., -1][want[..., -1] > 0].min())
    print(f"\n{name}: sim e_ref {e_ref:.3g} (at most {(D + 8) * 2.0 ** -24 * d2half:.3g}), fp32 numpy vs float64 {err:.3g}, bound {_bound(e_ref, 1.0):.3g}")
    assert e_ref <= (D + 8) * 2.0 ** -24 * d2half
    assert err <= _bound(e_ref, 1.0)
    assert (want[..., -1] == 1.0).any() and ((want[..., -1] > 0.999) & (want[..., -1] < 1.0)).any()      # an exact match; the near-duplicate


def test_colouring_edge_tiles():
    """the tiles the issue's edge segments must give, read off the reference's fixture"""
    name = "deeptile_default"
    c, t = deeptile_case.load(name), deeptile_case.load(name)["tiles"]
    emb, q = deeptile_case.embeddings(name), deeptile_case.load(name)["query"]
    B, Q = q.shape
    assert t[0, 0, 0, 0] == 3 and t[0, 0, 0, 1] == c["query_idf"][0, 0] and t[0, 0, 0, 2] == 1.0       # three occurrences
    for i in range(Q):                                                                                   # the empty-string segment: the zero row
        assert t[0, i, 2, 0] == 0 and t[0, i, 2, 1] == 0
        assert abs(t[0, i, 2, 2] - np.exp(-(emb[q[0, i]].astype(np.float64) ** 2).sum() / 2)) < 1e-6
    assert not t[0, :, 5].any()                                                                          # only literal pad tokens
    assert 0.999 < t[0, Q - 1, 6, 2] < 1.0 and t[0, Q - 1, 6, 0] == 0                                    # the near-duplicate row, tf 0
    assert not t[B - 1].any() and not t[1, Q - 1].any()                                                  # pad query terms
    assert not t[2, :, t.shape[2] // 2:].any() and t[2, 0, :t.shape[2] // 2, 2].all()                    # pad segments


def test_save_and_load_weights_round_trip(tmp_path):
    r, m = _model("deeptile_default")
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    fn = os.path.join(tmp_path, "w", "weights")
    r.save_weights(fn, opt)
    r2 = DeepTileBar(deeptile_case.config("deeptile_default"), deeptile_case.extractor("deeptile_default"))
    m2 = r2.build_model()
    for p in m2.parameters():
        p.data.zero_()
    r2.load_weights(fn, torch.optim.Adam(m2.parameters(), lr=1e-3))
    a, b = m.state_dict(), m2.state_dict()
    assert set(a) == set(b) and len(a) == 66
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_what_cannot_run_is_refused():
    ex = deeptile_case.extractor("deeptile_default")

    def with_config(**kw):
        e = deeptile_case.extractor("deeptile_default")
        e.config = dict(e.config, **kw)
        return e

    for cfg in ({"numberfilter": 2}, {"numberfilter": 4}, {"lstmhiddendim": 17}, {"lstmhiddendim": 0}, {"linearhiddendim1": 129}, {"linearhiddendim2": 129}):
        with pytest.raises(ValueError):
            DeepTileBar(cfg, ex).build_model()
    for kw in ({"passagelen": 9}, {"passagelen": 65}, {"maxqlen": 33}, {"maxqlen": 0}, {"tilechannels": 4}, {"tilechannels": 1}):
        with pytest.raises(ValueError):
            DeepTileBar({}, with_config(**kw)).build_model()
    from types import SimpleNamespace

    with pytest.raises(ValueError):
        DeepTileBar({}, SimpleNamespace(embeddings=ex.embeddings, config={})).build_model()
    # a tile tensor that disagrees with the model, at the call
    m = DeepTileBar({}, ex).build_model()
    for shape in ((2, 5, 20, 3), (2, 4, 20, 2), (2, 4, 9, 3), (2, 4, 65, 3), (2, 4, 20, 4), (4, 20, 3)):
        with pytest.raises(ValueError):
            m._forward_aten(torch.zeros(shape))
    assert m._forward_aten(torch.zeros(2, 1, 4, 10, 3)).shape == (2,)
    assert m._forward_aten(torch.zeros(2, 4, 64, 3)).shape == (2,)
    # the reranker's passagelen (30) is overridden by the extractor's, as in the reference
    assert m.p["passagelen"] == 20 and DeepTileBar({}, with_config(passagelen=64)).build_model().p["passagelen"] == 64


def test_abi_declares_binds_exports_and_refuses():
    from capreolus_amd import _lib

    lib = _lib.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "capreolus_amd.h")).read()
    for name in ("capamd_deeptile_color", "capamd_deeptile_forward", "capamd_deeptile_packed_floats"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "capamd_deeptile_model" in header and "#define CAPAMD_VERSION 405" in header and "#define CAPAMD_STATUS_SEGMENT_RANGE 128" in header
    assert _lib.VERSION == 405 and lib.capamd_version() == 405 and _lib.STATUS_SEGMENT_RANGE == 128
    P = 0x10000

    def model(**kw):
        m = _lib.DeepTileModel()
        m.packed, m.maxqlen, m.channels, m.filters, m.hidden, m.lin1, m.lin2 = P, 4, 3, 3, 3, 32, 16
        for k, v in kw.items():
            setattr(m, k, v)
        if "packed_floats" not in kw:
            m.packed_floats = max(lib.capamd_deeptile_packed_floats(ctypes.byref(m)), 0)
        return m

    # the packed size is the sum of the reference's parameter sizes
    _, net = _model("deeptile_default")
    assert lib.capamd_deeptile_packed_floats(ctypes.byref(model())) == sum(p.numel() for p in net.parameters())
    _, net = _model("deeptile_wide")
    assert lib.capamd_deeptile_packed_floats(ctypes.byref(model(maxqlen=32, hidden=16, lin1=128, lin2=128))) == sum(p.numel() for p in net.parameters())
    fwd = lambda m, B=8, Q=4, Pn=20, C=3: lib.capamd_deeptile_forward(P, B, Q, Pn, C, ctypes.byref(m), P, None, None)      # noqa: E731
    assert fwd(model(), B=0) == _lib.OK
    for mkw in ({"filters": 2}, {"filters": 4}, {"maxqlen": 0}, {"maxqlen": 33}, {"channels": 1}, {"channels": 4}, {"hidden": 0}, {"hidden": 17},
                {"lin1": 0}, {"lin1": 129}, {"lin2": 0}, {"lin2": 129}):
        m = model(**mkw)
        assert lib.capamd_deeptile_packed_floats(ctypes.byref(m)) == -1, mkw
        assert fwd(m, Q=m.maxqlen, C=m.channels) == _lib.ERR_ARG, mkw
    for skw in ({"Pn": 9}, {"Pn": 65}, {"Q": 5}, {"C": 2}, {"B": -1}):
        assert fwd(model(), **skw) == _lib.ERR_ARG, skw
    assert fwd(model(packed_floats=100)) == _lib.ERR_ARG and fwd(model(packed=None)) == _lib.ERR_ARG
    assert lib.capamd_deeptile_packed_floats(None) == -1
    assert lib.capamd_deeptile_forward(None, 8, 4, 20, 3, ctypes.byref(model()), P, None, None) == _lib.ERR_ARG
    assert lib.capamd_deeptile_forward(P, 8, 4, 20, 3, None, P, None, None) == _lib.ERR_ARG
    assert lib.capamd_deeptile_forward(P, 8, 4, 20, 3, ctypes.byref(model()), None, None, None) == _lib.ERR_ARG
    # the colouring: null pointers (every one but the stream) and each limit
    ok = [P, P, P, P, 8, 4, 96, 20, P, 1000, 300, 3, P, P, None]
    assert lib.capamd_deeptile_color(*(ok[:4] + [0] + ok[5:])) == _lib.OK
    for i in (0, 1, 2, 3, 8, 12, 13):
        args = list(ok)
        args[i] = None
        assert lib.capamd_deeptile_color(*args) == _lib.ERR_ARG, i
    for i, v in ((4, -1), (5, 0), (5, 33), (6, 0), (7, 0), (7, 65), (9, 0), (10, 0), (10, 513), (11, 1), (11, 4)):
        args = list(ok)
        args[i] = v
        assert lib.capamd_deeptile_color(*args) == _lib.ERR_ARG, (i, v)


def _restated(name, dtype=torch.float32):
    c = deeptile_case.load(name)
    _, m = _model(name)
    m.eval()
    with torch.no_grad():
        score, ev = m._forward_aten(torch.from_numpy(c["tiles"]), dtype=dtype, return_evidence=True)
    return c, score.numpy(), ev.numpy()


@pytest.mark.parametrize("name", deeptile_case.SCORE_CASES)
def test_restatement_matches_the_reference(name):
    c, s64, ev64 = _restated(name, torch.float64)
    _, score, ev = _restated(name)
    H = deeptile_case.config(name)["lstmhiddendim"]
    want_ev = c["evidence"].reshape(-1, 10, H)
    assert score.dtype == np.float32 and s64.dtype == np.float64 and ev.shape == want_ev.shape
    e_s, e_ev = float(np.abs(c["score"] - s64).max()), float(np.abs(want_ev - ev64).max())
    b_s, b_ev = _bound(e_s, np.abs(s64).max()), _bound(e_ev, np.abs(ev64).max())
    err = [np.abs(score - s64).max(), np.abs(score - c["score"]).max(), np.abs(ev - ev64).max(), np.abs(ev - want_ev).max()]
    print(f"\n{name}: scores e_ref {e_s:.3g} bound {b_s:.3g} fp32-vs-f64 {err[0]:.3g} fp32-vs-fixture {err[1]:.3g}; "
          f"W1 input e_ref {e_ev:.3g} bound {b_ev:.3g} fp32-vs-f64 {err[2]:.3g} fp32-vs-fixture {err[3]:.3g}")
    assert 0 < e_s <= 1e-5 * np.abs(s64).max()               # the reference's own fp32 error: small, and not zero
    assert err[0] <= b_s and err[1] <= b_s and err[2] <= b_ev and err[3] <= b_ev
    assert np.all(np.isfinite(score))
    assert score.max() - score.min() > 1000 * b_s             # the scores of a case spread over many error bounds


def test_restatement_gradients_match_the_reference():
    c = deeptile_case.load("deeptile_grad")
    r, m = _model("deeptile_grad")
    m.train()
    pos, neg = r.score({"posdoc": torch.from_numpy(c["tiles"])[:, None], "negdoc": torch.from_numpy(c["neg_tiles"])[:, None]})
    assert pos.requires_grad and neg.requires_grad
    score = torch.cat([pos, neg])
    np.testing.assert_allclose(score.detach().numpy(), c["score"], rtol=1e-5, atol=1e-5 * np.abs(c["score"]).max())
    (score * torch.from_numpy(c["loss_coef"])).sum().backward()
    names = [k[len("grad."):] for k in c if k.startswith("grad.")]
    assert set(names) == {k for k, p in m.named_parameters()} and len(names) == 66
    params = dict(m.named_parameters())
    for k in names:
        want, got = c["grad." + k], params[k].grad.numpy()
        assert np.abs(got - want).max() <= 1e-4 * max(np.abs(want).max(), 1e-6), (k, np.abs(got - want).max(), np.abs(want).max())


def test_a_batch_equals_its_documents_one_by_one():
    c = deeptile_case.load("deeptile_default")
    _, m = _model("deeptile_default")
    m.eval()
    t = torch.from_numpy(c["tiles"])
    with torch.no_grad():
        whole = m._forward_aten(t)
        single = torch.cat([m._forward_aten(t[i:i + 1]) for i in range(t.shape[0])])
    np.testing.assert_allclose(single.numpy(), whole.numpy(), rtol=1e-5, atol=1e-5 * float(whole.abs().max()))


def test_scoring_without_a_device_is_an_error_not_a_fallback():
    c = deeptile_case.load("deeptile_min")
    r, m = _model("deeptile_min")
    m.eval()
    with torch.no_grad(), pytest.raises(RuntimeError):
        r.test({"posdoc": torch.from_numpy(c["tiles"])[:, None]})
