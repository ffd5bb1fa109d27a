"""CEDR-KNRM's own device code against float64: the similarity tap (csrc/cedr_tap.h: cedr_pool_kernel, cedr_pool_cm_kernel<T, false>,
cedr_pool_cm_kernel<T, true>) through capamd_cedr_pool and the document head (csrc/cedr.hip) through capamd_cedr_score, on inputs of the
test's choosing.  The oracle is tests/cedr_case.py (pinned to the reference by tests/test_cedr_cpu.py), evaluated on the device.  Every
tap call prefills the output of all NP passages with NaN: rows p0 .. p0 + np must come back finite and within the bound, every other
row untouched."""
import ctypes

import numpy as np
import pytest
import torch

from capreolus_amd import _lib
from tests import cedr_case
from tests.cedr_case import SUPPORTED_LENGTHS, make_case, passage_masks, ref_pk, ref_score, ref_sims, to_cm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"fp16": (torch.float16, 1), "bf16": (torch.bfloat16, 0)}
LAYOUTS = {"rowmajor": 0, "chunkmajor": 1, "chunkmajor_ln": 2}
NAN_BITS = 0x7FC00000
LDS_LIMIT = 160 * 1024

# The bound.  The operands are exact (layout 2: tests/cedr_case.ln16 restates the kernel's LayerNorm bit for bit) and products of two
# 16-bit values are exact in fp32, so the kernel's error is the fp32 accumulation of the dot products and norms, the division and
# v_exp_f32.  |d/ds exp(-(s - mu)^2 / 2 sigma^2)| <= exp(-1/2) / sigma = 0.607 / sigma, so with a similarity error of at most DELTA
#     |got[k][a] - ref[k][a]| <= n_cols * (0.607 / sigma_k) * DELTA + 4e-7 * ref[k][a],      n_cols = the passage's live document columns.
# DELTA = 4 x the largest similarity error of a plain fp32 torch restatement (x.float() bmm, fp32 norms, ref_sims in fp32) against the
# float64 similarities over all cases of the geometry table, the random draws and the mask cases (the MFMA chain and torch sum in
# different orders; 4 x is what TK's kernels needed of theirs, 3.7 x).
# Measured on an MI355X over those 126 calls: the restatement's largest error is 2.861e-6 (bf16, H = 768, S = 256; fp16 1.79e-6 - torch
# adds the 768..1024 products of a dot product one rounding each, and the squared norms are sums of positive terms).  The kernels need
# far less than the restatement: the similarity error that explains their worst sum, as a fraction of RESTATEMENT_ERR, is
#     row-major fp16 0.006, bf16 0.004;  chunk-major fp16 0.016, bf16 0.016;  chunk-major + LayerNorm fp16 0.053, bf16 0.053
# (1.5e-7 at most: the MFMA adds 16 products per rounding of the accumulator).  4 x is therefore generous here, and it is not raised.
RESTATEMENT_ERR = 2.861e-6
DELTA = 4 * RESTATEMENT_ERR


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call_pool(c, **over):
    """capamd_cedr_pool on a case (tests/cedr_case.make_case), keyword arguments replacing single arguments -> (rc, out [NP, K, A])"""
    a = dict(xin=c["xin"], layout=c["layout"], mr=c["mr"], gamma=c["gamma"], beta=c["beta"], mask=c["mask"], seg=c["seg"], qmask0=c["qmask0"],
             p0=c["p0"], n=c["n"], NP=c["NP"], S=c["S"], H=c["H"], maxqlen=c["A"] - 1, mu=c["mu"], sigma=c["sigma"], K=c["K"],
             code=1 if c["dtype"] == torch.float16 else 0)
    a.update(over)
    out = over.get("out")
    if out is None:
        out = torch.full((c["NP"], c["K"], c["A"]), float("nan"), dtype=torch.float32, device=DEV)
    rc = _lib.load().capamd_cedr_pool(_p(a["xin"]), a["layout"], _p(a["mr"]), _p(a["gamma"]), _p(a["beta"]), _p(a["mask"]), _p(a["seg"]),
                                      _p(a["qmask0"]), a["p0"], a["n"], a["NP"], a["S"], a["H"], a["maxqlen"], _p(a["mu"]), _p(a["sigma"]),
                                      a["K"], _p(out), a["code"], _stream())
    torch.cuda.synchronize()
    return rc, out


def untouched(out, lo, hi):
    """every row of out outside lo .. hi still holds the prefilled NaN, bit for bit"""
    bits = out.view(torch.int32)
    return bool((bits[:lo] == NAN_BITS).all()) and bool((bits[hi:] == NAN_BITS).all())


def bound_of(c, ref, delta):
    _, dmask, _ = ref_sims(c["x"], c["mask"], c["seg"], c["A"])
    n_cols = dmask.sum(dim=1).view(-1, 1, 1)
    return n_cols * (0.607 / c["sigma"].double().view(1, -1, 1)) * delta + 4e-7 * ref


def figures(c, out):
    """(largest similarity error of the fp32 torch restatement, the similarity error the kernel's sums need under the bound) of a call"""
    s64, dmask, _ = ref_sims(c["x"], c["mask"], c["seg"], c["A"])
    s32, _, _ = ref_sims(c["x"], c["mask"], c["seg"], c["A"], dtype=torch.float32)
    restate = (s32.double() - s64).abs().max().item()
    ref = ref_pk(c["x"], c["mask"], c["seg"], c["qmask0"][c["p0"]:c["p0"] + c["n"]], c["A"], c["mu"], c["sigma"])
    err = ((out[c["p0"]:c["p0"] + c["n"]].double() - ref).abs() - 4e-7 * ref).clamp(min=0)
    per = dmask.sum(dim=1).view(-1, 1, 1).clamp(min=1) * (0.607 / c["sigma"].double().view(1, -1, 1))
    return restate, (err / per).max().item()


def check_pool(c, what):
    rc, out = call_pool(c)
    assert rc == _lib.OK, (what, rc)
    p0, n = c["p0"], c["n"]
    assert untouched(out, p0, p0 + n), f"{what}: a row outside {p0}..{p0 + n} was written"
    got = out[p0:p0 + n].double()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    ref = ref_pk(c["x"], c["mask"], c["seg"], c["qmask0"][p0:p0 + n], c["A"], c["mu"], c["sigma"])
    restate, need = figures(c, out)
    print(f"CEDRTAP {what} restatement {restate:.3e} kernel needs {need:.3e}")
    over = (got - ref).abs() - bound_of(c, ref, DELTA)
    assert over.max().item() <= 0, (what, "worst excess", over.max().item(), "at", np.unravel_index(int(over.argmax()), over.shape),
                                    "similarity error needed", need, "allowed", DELTA)
    return out, ref


# ---- a. geometries ---------------------------------------------------------------------------------------------------------------
# id: (S, H chunk-major, H row-major, A, K, np, p0).  tpr = min(256 / A, 32) threads pool one query row.
GEOMETRY = {
    "one_tile_idle_waves": (32, 256, 64, 2, 1, 1, 0),            # three of four waves own no tile; tpr clamp at 32 with 192 threads idle
    "benchmark": (256, 768, 768, 13, 11, 8, 0),
    "lds_maximum": (512, 1024, 1024, 32, 11, 3, 2),             # 154,464 bytes of LDS, all 32 rows of the MFMA tile live
    "tpr_clamp": (96, 512, 512, 8, 10, 5, 0),                    # rows 8..31 of the tile dead; 3 tiles: wave 3 idle
    "tpr_28": (160, 256, 256, 9, 11, 4, 1),                      # 252 live threads; two trips per tile
    "tpr_12": (384, 768, 768, 21, 2, 2, 0),
    "tiles_not_4n": (224, 512, 512, 13, 11, 9, 3),               # 7 tiles over 4 waves
    "rowmajor_h128": (64, None, 128, 13, 11, 15, 0),             # the widths of the mini fixtures: row-major only
    "rowmajor_h192": (128, None, 192, 9, 11, 15, 0),
}
GEOMETRY_PARAMS = [(g, lay) for g in GEOMETRY for lay in LAYOUTS if not (GEOMETRY[g][1] is None and lay != "rowmajor")]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("geom,layout", GEOMETRY_PARAMS)
def test_tap_geometry(geom, layout, dt):
    S, Hcm, Hrm, A, K, n, p0 = GEOMETRY[geom]
    c = make_case(S, Hrm if layout == "rowmajor" else Hcm, A, K, n, p0=p0, NP=p0 + n + 2, seed=sum(map(ord, geom)), dtype=DTYPES[dt][0],
                  layout=LAYOUTS[layout], device=DEV)
    check_pool(c, f"{geom} {layout} {dt}")


def _draw(layout, i):
    rs = np.random.RandomState(9000 + 100 * LAYOUTS[layout] + i)
    S = int(rs.choice(SUPPORTED_LENGTHS))
    H = int(rs.choice(np.arange(64, 1025, 64))) if layout == "rowmajor" else int(rs.choice([256, 512, 768, 1024]))
    A = int(rs.randint(2, min(32, S - 1) + 1))
    return S, H, A, int(rs.randint(1, 12)), int(rs.randint(1, 7)), int(rs.randint(0, 4))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("i", range(12))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_tap_random_geometry(layout, i, dt):
    S, H, A, K, n, p0 = _draw(layout, i)
    c = make_case(S, H, A, K, n, p0=p0, NP=p0 + n + 1, seed=500 + i, dtype=DTYPES[dt][0], layout=LAYOUTS[layout], device=DEV)
    what = f"draw {i} S {S} H {H} A {A} K {K} np {n} p0 {p0} {layout} {dt}"
    # (inside the entry point's other limits the chunk-major kernels peak at 154,464 bytes - S 512, H 1024, A 32 - so no draw is refused
    # for LDS; the branch stays in case a limit moves)
    if layout != "rowmajor" and cedr_case.cm_lds_bytes(S, H, A) > LDS_LIMIT:
        rc, out = call_pool(c)
        assert rc == _lib.ERR_ARG and untouched(out, 0, 0), what
        return
    check_pool(c, what)


# ---- b. masks --------------------------------------------------------------------------------------------------------------------
def _mask_case(S, H, A, layout, dt):
    """One call, one passage per mask situation -> (case, names, passages whose sums must be exactly 0)"""
    full = S - (A + 3) - 3
    rows = [("query of length 1", passage_masks(S, 1, S // 2)),
            ("query of length A - 1: [SEP] is the last query row", passage_masks(S, A - 1, full)),
            ("query of length A + 3: its tail is neither row nor column", passage_masks(S, A + 3, full)),
            ("document starts inside the query rows and runs to the last column", passage_masks(S, 2, S - 5)),
            ("holes in the attention mask", passage_masks(S, A - 2, full)),
            ("nothing attended", (np.zeros(S, dtype=np.int64), passage_masks(S, 3, 9)[1])),
            ("no segment-1 token", (passage_masks(S, 5, 9)[0], np.zeros(S, dtype=np.int64))),
            ("qmask0 all ones over a short query", passage_masks(S, 2, full)),
            ("qmask0 all zeros over a full query", passage_masks(S, A, full)),
            ("all-zero hidden row at a query row", passage_masks(S, A, full)),
            ("all-zero hidden row at a document column", passage_masks(S, 4, full))]
    names, masks = [r[0] for r in rows], [(r[1][0].copy(), r[1][1].copy()) for r in rows]
    masks[4][0][2] = 0                       # a query row ...
    masks[4][0][A + 4] = 0                   # ... and a document column (the document starts at A)
    zero_rows = [(9, 2), (10, 4 + 2 + 3)]
    n = len(rows)
    c = make_case(S, H, A, 11, n, p0=1, NP=n + 2, seed=S + H, dtype=DTYPES[dt][0], layout=LAYOUTS[layout], device=DEV, masks=masks,
                  zero_rows=zero_rows)
    own = ((c["mask"][:, 1:A + 1] != 0) & (c["seg"][:, 1:A + 1] == 0)).float()          # what the engine hands in for a first passage
    c["qmask0"] = torch.zeros((c["NP"], A), device=DEV)
    c["qmask0"][1:1 + n] = own
    c["qmask0"][1 + 7] = 1
    c["qmask0"][1 + 8] = 0
    c["mu"] = torch.tensor([-0.9, -0.7, -0.5, -0.3, -0.1, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0], device=DEV)     # the reference's bank (exact match last)
    c["sigma"] = torch.tensor([0.1] * 10 + [0.01], device=DEV)
    return c, names, (5, 6, 8)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("S,H,A", [(64, 256, 9), (256, 768, 13)])
def test_tap_masks(S, H, A, layout, dt):
    c, names, zero = _mask_case(S, H, A, layout, dt)
    rc, out = call_pool(c)
    assert rc == _lib.OK and untouched(out, 1, 1 + c["n"])
    ref = ref_pk(c["x"], c["mask"], c["seg"], c["qmask0"][1:1 + c["n"]], A, c["mu"], c["sigma"])
    restate, need = figures(c, out)
    print(f"CEDRTAP masks S {S} {layout} {dt} restatement {restate:.3e} kernel needs {need:.3e}")
    got, bound = out[1:1 + c["n"]].double(), bound_of(c, ref, DELTA)
    assert ref[9].abs().max() > 0 and ref[10].abs().max() > 0 and ref[3, :, :3].abs().max() > 0       # (the cases are what they say)
    assert ref[2, 5].min() > 0 and ref[1, 5, A - 1] > 0
    for p, name in enumerate(names):
        assert bool(torch.isfinite(got[p]).all()), name
        if p in zero:
            assert ref[p].abs().max().item() == 0 and got[p].abs().max().item() == 0, name
        over = ((got[p] - ref[p]).abs() - bound[p]).max().item()
        assert over <= 0, (name, over, need, DELTA)


# ---- c. the three layouts on one hidden state ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("S,H,A,K,n", [(64, 256, 9, 11, 5), (256, 768, 13, 11, 4), (512, 1024, 32, 7, 2)])
def test_tap_layouts_agree(S, H, A, K, n, dt):
    """layout 2 with mu = 0, rstd = 1, gamma = 1, beta = 0 normalises to the stored value itself, so the two chunk-major kernels run
    the same instructions on equal operands: bit for bit.  The row-major kernel holds the query operand in registers instead of LDS
    and walks k in steps of 64 instead of 128; it accumulates in the same order and has been bit-equal wherever measured, but only
    the bound is asserted of it (once: both are compared with each other, not each with the reference)."""
    c = make_case(S, H, A, K, n, NP=n, seed=77 + S, dtype=DTYPES[dt][0], layout=2, device=DEV, unit_ln=True)
    flat = c["x"].reshape(n * S, H)
    assert torch.equal(flat, cedr_case.from_cm(c["xin"], n * S, H))                # ln16 returned the stored values
    out2, ref = check_pool(c, f"layouts agree S {S} chunkmajor_ln {dt}")
    rc1, out1 = call_pool(c, layout=1, mr=None, gamma=None, beta=None)
    rc0, out0 = call_pool(c, layout=0, mr=None, gamma=None, beta=None, xin=flat.reshape(-1).contiguous())
    assert rc1 == _lib.OK and rc0 == _lib.OK
    assert torch.equal(out1.view(torch.int32), out2.view(torch.int32))
    print("CEDRTAP layouts", S, H, dt, "row-major bit-equal to chunk-major:", torch.equal(out0, out1))
    assert ((out0.double() - out1.double()).abs() - bound_of(c, ref, DELTA)).max().item() <= 0


# ---- d. micro-batch placement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_tap_microbatch_placement(layout, dt):
    """one call over 9 passages == nine calls of one passage at p0 = 0..8 (a passage is one workgroup; p0 only moves qmask0 / the output)"""
    S, H, A, K, n = 96, 256, 11, 11, 9
    c = make_case(S, H, A, K, n, NP=n, seed=31, dtype=DTYPES[dt][0], layout=LAYOUTS[layout], device=DEV)
    whole, _ = check_pool(c, f"placement {layout} {dt}")
    parts = torch.full((n, K, A), float("nan"), dtype=torch.float32, device=DEV)
    for p in range(n):
        rc, _ = call_pool(c, xin=c["xin"][p * S * H:(p + 1) * S * H], mr=None if c["mr"] is None else c["mr"][p * S:(p + 1) * S],
                          mask=c["mask"][p:p + 1], seg=c["seg"][p:p + 1], p0=p, n=1, out=parts)
        assert rc == _lib.OK
        assert untouched(parts, 0, p + 1)
    assert torch.equal(whole.view(torch.int32), parts.view(torch.int32))


# ---- f. refusals ----------------------------------------------------------------------------------------------------------------
REFUSALS = {
    "hidden not a multiple of 64": (0, dict(H=96), _lib.ERR_ARG),
    "hidden below 64": (0, dict(H=32), _lib.ERR_ARG),
    "hidden above 1024": (0, dict(H=1088), _lib.ERR_ARG),
    "hidden above 1024, chunk-major": (1, dict(H=1280), _lib.ERR_ARG),
    "S = 48": (0, dict(S=48), _lib.ERR_ARG),
    "S = 288": (1, dict(S=288), _lib.ERR_ARG),
    "S = 16": (0, dict(S=16), _lib.ERR_ARG),
    "maxqlen + 1 > 32": (0, dict(maxqlen=32), _lib.ERR_ARG),
    "maxqlen + 2 > S": (0, dict(S=32, maxqlen=31), _lib.ERR_ARG),
    "maxqlen = 0": (0, dict(maxqlen=0), _lib.ERR_ARG),
    "K = 0": (0, dict(K=0), _lib.ERR_ARG),
    "K = 12": (2, dict(K=12), _lib.ERR_ARG),
    "p0 + np > NP": (0, dict(p0=2), _lib.ERR_ARG),
    "np = 0": (0, dict(n=0), _lib.ERR_ARG),
    "negative p0": (1, dict(p0=-1), _lib.ERR_ARG),
    "chunk-major with hidden % 256 != 0": (1, dict(H=192), _lib.ERR_ARG),
    "chunk-major LayerNorm with hidden % 256 != 0": (2, dict(H=128), _lib.ERR_ARG),
    "layout 2 without statistics": (2, dict(mr=None), _lib.ERR_ARG),
    "layout 2 without gamma": (2, dict(gamma=None), _lib.ERR_ARG),
    "layout 2 without beta": (2, dict(beta=None), _lib.ERR_ARG),
    "layout 3": (0, dict(layout=3), _lib.ERR_ARG),
    "dtype 2": (0, dict(code=2), _lib.ERR_ARG),
    "no mask": (0, dict(mask=None), _lib.ERR_ARG),
    "no kernel means": (0, dict(mu=None), _lib.ERR_ARG),
    "x two bytes off": (0, "shift1", _lib.ERR_ALIGN),
    "x eight bytes off, chunk-major": (1, "shift4", _lib.ERR_ALIGN),
    "x eight bytes off, chunk-major LayerNorm": (2, "shift4", _lib.ERR_ALIGN),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_tap_refusals(name):
    layout, over, want = REFUSALS[name]
    c = make_case(64, 256, 9, 11, 3, p0=1, NP=4, seed=3, dtype=torch.float16, layout=layout, device=DEV)
    if isinstance(over, str):
        k = int(over[5:])
        pad = torch.zeros(c["xin"].numel() + 8, dtype=c["xin"].dtype, device=DEV)
        pad[k:k + c["xin"].numel()] = c["xin"]
        over = dict(xin=pad[k:k + c["xin"].numel()])
        assert over["xin"].data_ptr() % 16 == 2 * k
    rc, out = call_pool(c, **over)
    assert rc == want, (name, rc)
    assert untouched(out, 0, 0), name
    rc, out = call_pool(c)                                     # and the call it was derived from is served
    assert rc == _lib.OK and untouched(out, 1, 4) and bool(torch.isfinite(out[1:4]).all())


def test_tap_lds_limit_is_out_of_reach():
    """the 160 KiB refusal of the chunk-major kernels cannot be provoked inside the other limits: their largest need is served (the
    lds_maximum row of the geometry table)"""
    assert max(cedr_case.cm_lds_bytes(S, 1024, 32) for S in SUPPORTED_LENGTHS) == 154464 <= LDS_LIMIT


# ---- g. the document head alone ---------------------------------------------------------------------------------------------------
def _score_case(P, cls_mode, n_layers, A, K, combine_hidden, hidden=64, B=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    NP = B * P
    pk = torch.pow(10.0, 5 * torch.rand((max(n_layers, 1), NP, K, A), generator=g) - 3)         # 1e-3 .. 1e2
    # document 0: a query row no passage matches (the clamp), sums below the clamp, very large sums
    pk[:, :P, 0, 0] = 0
    pk[:, :P, K - 1, A - 1] = 1e-30
    pk[:, P - 1, 0, A - 1] = 1e30
    if B > 1:
        pk[0, P:2 * P, :, 0] = 0                            # document 1: the first query row dead in every kernel of the first layer
    cls = torch.randn((NP, hidden), generator=g)
    cls[:, ::2] -= 6                                        # every other column negative in all passages (a max that starts from 0 shows)
    n_in = (hidden if cls_mode else 0) + n_layers * K
    w1 = torch.randn((combine_hidden or 1, n_in), generator=g) * 0.3
    b1 = torch.randn((combine_hidden or 1,), generator=g) * 0.1
    w2 = torch.randn((combine_hidden,), generator=g) * 0.3 if combine_hidden else None
    b2 = torch.randn((1,), generator=g) * 0.1 if combine_hidden else None
    return [None if t is None else t.to(DEV) for t in (pk, cls, w1, b1, w2, b2)] + [n_in]


def _check_score(P, cls_mode, n_layers, A, K, combine_hidden, hidden=64, B=4, seed=0):
    pk, cls, w1, b1, w2, b2, n_in = _score_case(P, cls_mode, n_layers, A, K, combine_hidden, hidden, B, seed)
    out = torch.full((B,), float("nan"), device=DEV)
    feats = torch.full((B, n_in), float("nan"), device=DEV)
    rc = _lib.load().capamd_cedr_score(_p(pk), _p(cls), B, P, A - 1, n_layers, K, hidden, cls_mode, _p(w1), _p(b1), combine_hidden, _p(w2), _p(b2),
                                       _p(out), _p(feats), _stream())
    torch.cuda.synchronize()
    what = (P, cls_mode, n_layers, A, K, combine_hidden, hidden)
    assert rc == _lib.OK, what
    want, wf = ref_score(pk[:n_layers] if n_layers else None, cls, P, cls_mode, w1 if combine_hidden else w1.view(-1), b1, w2, b2)
    assert bool(torch.isfinite(feats).all()) and bool(torch.isfinite(out).all()), what
    ef = ((feats.double() - wf).abs() - 1e-6 * wf.abs().clamp(min=1)).max().item()
    es = (out.double() - want).abs().max().item()
    assert ef <= 0, (what, "feature excess", ef)
    assert es <= 1e-5 * max(1.0, want.abs().max().item()), (what, es, want.abs().max().item())


@pytest.mark.parametrize("combine_hidden", [0, 1, 32, 2048])
@pytest.mark.parametrize("n_layers", [0, 1, 13])
@pytest.mark.parametrize("cls_mode", [0, 1, 2])
@pytest.mark.parametrize("P", [1, 3, 8])
def test_score_alone(P, cls_mode, n_layers, combine_hidden):
    if cls_mode == 0 and n_layers == 0:             # no feature at all: refused (CEDRKNRM_Class.forward raises on this configuration)
        pk, cls, w1, b1, w2, b2, _ = _score_case(P, 1, 0, 13, 11, combine_hidden)
        out = torch.full((4,), float("nan"), device=DEV)
        rc = _lib.load().capamd_cedr_score(_p(pk), _p(cls), 4, P, 12, 0, 11, 64, 0, _p(w1), _p(b1), combine_hidden, _p(w2), _p(b2), _p(out), None, _stream())
        torch.cuda.synchronize()
        assert rc == _lib.ERR_ARG and bool(torch.isnan(out).all())
        return
    for A in (2, 13, 32):
        for K in (1, 11):
            _check_score(P, cls_mode, n_layers, A, K, combine_hidden, seed=A * K + P)


@pytest.mark.parametrize("combine_hidden", [0, 2048])
def test_score_at_the_input_limit(combine_hidden):
    """n_in = 2048 exactly: a 1024-wide [CLS] feature and 1024 kernel features (13 hidden states x 11 kernels is 143; 128 x 8 fills the
    rest of the feature buffer), and one more is refused - by a wider [CLS] row and by one more hidden state"""
    _check_score(3, 1, 128, 13, 8, combine_hidden, hidden=1024, B=3, seed=9)
    _check_score(2, 2, 13, 13, 11, combine_hidden, hidden=1024, B=3, seed=10)
    for n_layers, hidden in ((128, 1025), (129, 1024)):
        pk, cls, w1, b1, w2, b2, n_in = _score_case(3, 1, n_layers, 13, 8, combine_hidden, hidden=hidden, B=3)
        assert n_in > 2048
        out = torch.full((3,), float("nan"), device=DEV)
        rc = _lib.load().capamd_cedr_score(_p(pk), _p(cls), 3, 3, 12, n_layers, 8, hidden, 1, _p(w1), _p(b1), combine_hidden, _p(w2), _p(b2), _p(out),
                                           None, _stream())
        torch.cuda.synchronize()
        assert rc == _lib.ERR_ARG and bool(torch.isnan(out).all())


# ---- h. the features of the BERT-base fixture, per hidden state ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_features():
    from oracle import bert_port
    from tests.helpers import load_cedr_case

    c, w, head, mus, sigmas = load_cedr_case("base")
    d = [torch.from_numpy(c[k].astype(np.int64)) for k in ("pos_bert_input", "pos_mask", "pos_seg")]
    n_in = head["combine.0.weight"].shape[1]
    eye = {"combine.0.weight": torch.eye(n_in), "combine.0.bias": torch.zeros(n_in)}       # the port with an identity head returns the features
    want = bert_port.cedr_knrm(w, eye, *d, int(c["dims"][2]), int(c["dims"][1]), int(c["maxqlen"]), [int(x) for x in c["simmat_layers"]], mus, sigmas,
                               c["cls_mode"])
    return c, w, head, d, want.view(d[0].shape[0], n_in).numpy()


@pytest.mark.parametrize("skip_padding", [True, False])
def test_cedr_features_match_port_on_base(base_features, skip_padding):
    """test_cedr_features_match_port_on_mini's assertion where the chunk-major kernels run: BERT-base, fp16, 13 hidden states, each
    hidden state's 11 kernel features on their own (2e-3 of the largest kernel feature, the bound of the mini test)."""
    from tests.test_gpu_bert import _cedr_model

    c, w, head, d, want = base_features
    m = _cedr_model(c, w, head, "fp16", skip_padding).model
    dd = [t.to(DEV) for t in d]
    with torch.no_grad():
        m(*dd)
        mu, sigma = m.kernels.stacked()
        lin = m.combine[0]
        _, feats = m._engine.forward(*dd, int(c["maxqlen"]), m._layers, mu, sigma, c["cls_mode"], lin.weight.detach().contiguous(), lin.bias.detach(),
                                     m.combine[1].weight.detach().view(-1), m.combine[1].bias.detach(), return_features=True,
                                     skip_padding=skip_padding)
    got, H, K = feats.cpu().numpy(), int(c["dims"][0]), 11
    sel = [int(x) for x in c["simmat_layers"]]
    assert got.shape == want.shape == (d[0].shape[0], H + K * len(sel))
    assert np.abs(got[:, :H] - want[:, :H]).max() <= 2e-3 * np.abs(want[:, :H]).max()     # [CLS] rows of a 16-bit encoder
    scale = np.abs(want[:, H:]).max()
    errs = [np.abs(got[:, H + K * i:H + K * (i + 1)] - want[:, H + K * i:H + K * (i + 1)]).max() / scale for i in range(len(sel))]
    print("CEDRBASE skip_padding", skip_padding, "per hidden state, error / largest kernel feature:", " ".join(f"{li}:{e:.2e}" for li, e in zip(sel, errs)))
    bad = {li: e for li, e in zip(sel, errs) if not e <= 2e-3}
    assert not bad, f"hidden states over 2e-3 of the largest kernel feature: {bad}"
