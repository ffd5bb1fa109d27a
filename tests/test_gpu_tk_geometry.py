"""TK (csrc/tk.hip) over the geometries its three score fixtures never reach: every instantiation of attn_kernel<HS> (head slot 48, and
head widths that fill their slot), gemm_ln_kernel<CT> for every CT and for Dp == D, the ReLU GEMM's three tilings, the pooling's
later chunks of 8 query rows, whole 64-key tiles masked before the first live key, L = 1 and L = max_len, and a micro-batch of more
than 65,535 sequences in the attention grid's z.  The oracle is the float64 restatement (TK_class._forward_aten) on the device, which
test_tk_cpu.py pins against the reference; the bound is test_gpu_tk.py's."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from capreolus_amd import _lib, engine
from capreolus_amd.reranker import TK
from tests import tk_case
from tests.test_gpu_tk import _check_features

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _row(D, heads, ffdim, layers, Q, L, B=6, usemask=False, mixer=None, alpha=0.5, V=300, seed=0):
    return dict(D=D, heads=heads, ffdim=ffdim, layers=layers, Q=Q, L=L, B=B, usemask=usemask, mixer=mixer, alpha=alpha, V=V, seed=seed)


# head slot = head width rounded up to 16 (attn_kernel<HS>); Dp / 64 = gemm_ln_kernel<CT>; Fp / 64 picks the ReLU GEMM's CT (3 if
# divisible by 3, else 2 if even, else 1); Q > 8 runs pool_kernel's query staging more than once
ROWS = {
    # the smallest of everything: head slot 16 of width 2, ffdim 1, one query row, one key
    "d2_l1": _row(2, 1, 1, 1, Q=1, L=1, seed=1),
    # head width 64 = its slot (no pad columns); Dp == D for LayerNorm (nreal = the whole width); ReLU GEMM with CT 3; 3 layers;
    # Q = 9: a last pooling chunk of 1 row; L = 65: a second key tile of 1 key
    "d64_h1": _row(64, 1, 192, 3, Q=9, L=65, seed=2),
    # usemask + mixer: slot 32 filled; gemm_ln CT 2 with Dp == D; Q = 17; the dead-tile documents (keys 0..128 masked)
    "d128_mask": _row(128, 4, 256, 2, Q=17, L=130, B=8, usemask=True, mixer=0.6, seed=3),
    # head width 40 in slot 48; gemm_ln CT 4; ReLU GEMM CT 1 over 5 column blocks; Q = 12; alpha 0 (context only)
    "d200_hs48": _row(200, 5, 320, 2, Q=12, L=300, alpha=0.0, seed=4),
    # width 50 in slot 64 under usemask; gemm_ln CT 3; L = 64: exactly one key tile
    "d150_mask": _row(150, 3, 100, 1, Q=8, L=64, B=8, usemask=True, seed=5),
    # head width 48 = slot 48 (no pad columns) under usemask + mixer; gemm_ln CT 6; ReLU CT 3 twice; 4 layers; Q = 32 (4 full
    # chunks); L = 129: the first live key of the dead-tile document is alone in the third tile
    "d384_mask": _row(384, 8, 384, 4, Q=32, L=129, B=8, usemask=True, mixer=0.4, seed=6),
    # width 60 in slot 64; gemm_ln CT 7; ReLU CT 1 over 7 blocks; L = 127
    "d420_h7": _row(420, 7, 448, 1, Q=5, L=127, seed=7),
    # the widest: gemm_ln CT 8 with Dp == D; ReLU CT 2 x 4; Q = 31 (last chunk of 7)
    "d512_h8": _row(512, 8, 512, 2, Q=31, L=200, seed=8),
    # 512 heads of width 1 (slot 16, Hs = 8192: a 24576-wide QKV GEMM, 512 blocks in the attention grid's y)
    "d512_h512": _row(512, 512, 64, 1, Q=4, L=64, seed=9),
    # L = max_len: the last rows of pe, 79 key tiles (float64 attention is [B, H, L, L]: kept to 3 documents of 2 heads)
    "d50_l5000": _row(50, 2, 64, 1, Q=4, L=5000, B=3, seed=10),
}

WIDTHS = (2, 50, 64, 128, 150, 200, 384, 420, 512)
LENGTHS = (1, 7, 63, 64, 65, 128, 129, 300, 800)


def _random_row(seed):
    rs = np.random.RandomState(7000 + seed)
    D = int(rs.choice(WIDTHS))
    L = int(rs.choice(LENGTHS))
    usemask = bool(rs.rand() < 0.5)
    B = 8 if usemask else 6
    # head widths <= 64, and the float64 attention scores [B, H, L, L] within about 2 GB
    heads = [h for h in range(1, D + 1) if D % h == 0 and D // h <= 64 and B * h * L * L * 8 <= 2 << 30]
    mixer = float(np.round(rs.uniform(0.1, 0.9), 3)) if rs.rand() < 0.5 else None
    return _row(D, int(rs.choice(heads)), int(rs.randint(1, 513)), int(rs.randint(1, 5)), Q=int(rs.randint(1, 33)), L=L, B=B,
                usemask=usemask, mixer=mixer, alpha=float(rs.choice([0.0, 0.2, 0.5, 0.8])), seed=100 + seed)


def _geometry(row):
    return ", ".join(f"{k} {v}" for k, v in row.items())


def _make(row):
    """(plugin, fp32 model on the device, the float64 model on the device, query ids, document ids) of a row"""
    rs = np.random.RandomState(row["seed"])
    emb = tk_case.make_embeddings(rs, row["V"], row["D"])
    w = tk_case.make_weights(rs, row["D"], row["ffdim"], row["layers"], 0.9 if row["mixer"] is None else row["mixer"])
    q, d = tk_case.make_ids(rs, row["B"], row["Q"], row["L"], row["V"], mid_pads=True, dead_tiles=row["usemask"])
    cfg = dict(tk_case.DEFAULTS, numattheads=row["heads"], ffdim=row["ffdim"], numlayers=row["layers"], usemask=row["usemask"],
               usemixer=row["mixer"] is not None, alpha=row["alpha"])
    ex = SimpleNamespace(embeddings=emb, pad=0, config={"maxqlen": row["Q"], "maxdoclen": row["L"]})
    r, m = tk_case.build_from(cfg, ex, w, TK)
    m.to(DEV).eval()
    m64 = tk_case.build_from(cfg, ex, w, TK)[1].double().to(DEV).eval()
    return r, m, m64, torch.from_numpy(q).to(DEV), torch.from_numpy(d).to(DEV)


def _batch(q, d):
    return {"query": q, "posdoc": d, "query_idf": torch.zeros(q.shape, device=DEV)}


def _poison(m, q, d):
    """fill the engine's workspace for this call with 0xFF bytes (NaN floats), so that a kernel that reads a cell no kernel of the
    call wrote (the out-proj GEMM reading ctx's pad columns past the last head slot, say) gives NaN instead of what was left there"""
    with torch.no_grad():
        m.forward_engine(d, q)
    m._engine._ws.fill_(255)


def _check_row(row):
    r, m, m64, q, d = _make(row)
    _poison(m, q, d)
    with torch.no_grad():
        score, feats = m.forward_engine(d, q, features=True)
        test = r.test(_batch(q, d))
        s64, f64 = m64._forward_aten(d, q, return_features=True)
    assert torch.isfinite(s64).all(), _geometry(row)
    assert torch.isfinite(score).all(), _geometry(row)
    assert torch.equal(test, score), _geometry(row)
    try:
        _check_features(feats.cpu().numpy(), f64.cpu().numpy())
    except AssertionError as e:
        raise AssertionError(f"{_geometry(row)}: max error / max |feature| = {e}") from None


@pytest.mark.parametrize("name", list(ROWS))
def test_geometry_table_against_float64(name):
    _check_row(ROWS[name])


@pytest.mark.parametrize("seed", range(12))
def test_random_geometries_against_float64(seed):
    _check_row(_random_row(seed))


@pytest.mark.parametrize("name", ["d200_hs48", "d128_mask"])
def test_scores_do_not_depend_on_microbatch(name):
    r, m, _, q, d = _make(ROWS[name])
    b = _batch(q, d)
    _poison(m, q, d)
    with torch.no_grad():
        want = r.test(b)
        for nb in (1, 4, None):
            m._engine.docs_per_microbatch = nb
            assert torch.equal(r.test(b), want), nb
    assert torch.isfinite(want).all()


def test_microbatch_beyond_the_grid_z_limit():
    """The default micro-batch of short documents holds more than 65,535 sequences, one attention workgroup each in the grid's z.  The
    call of 70,000 equals the same documents scored 1,000 at a time."""
    row = _row(50, 5, 64, 1, Q=4, L=4, B=70000, seed=20)
    r, m, _, q, d = _make(row)
    eng = m._engine
    assert eng.docs_per_microbatch is None
    mod, keep = eng.model(m._params(), row["heads"], row["layers"], False, row["alpha"], 0, 1e-5)
    lib = _lib.load()
    one = lib.capamd_tk_workspace_bytes(ctypes.byref(mod), 1, row["Q"], row["L"])
    per_doc = lib.capamd_tk_workspace_bytes(ctypes.byref(mod), 2, row["Q"], row["L"]) - one
    nb = min(engine.TK_WORKSPACE_BUDGET // per_doc, row["B"])
    assert nb > 65535, (per_doc, nb)
    eng._ws = torch.full((lib.capamd_tk_workspace_bytes(ctypes.byref(mod), nb, row["Q"], row["L"]),), 255, dtype=torch.uint8, device=DEV)
    with torch.no_grad():
        whole = m.forward_engine(d, q)
        parts = torch.cat([m.forward_engine(d[i:i + 1000], q[i:i + 1000]) for i in range(0, row["B"], 1000)])
    assert torch.isfinite(whole).all()
    for lo, hi in ((0, 8), (65528, 65544), (69992, 70000)):
        assert torch.equal(whole[lo:hi], parts[lo:hi]), (lo, hi)
    assert torch.equal(whole, parts), (whole != parts).nonzero()[:8].flatten().tolist()


@pytest.mark.parametrize("side,pos,value", [("query", (0, 1), 300), ("posdoc", (2, 3), -1), ("query", (3, 0), -5), ("posdoc", (5, 7), 10 ** 6)])
def test_out_of_range_ids_raise_and_the_next_call_is_clean(side, pos, value):
    """a query id >= vocab, a negative document id, a negative query id, and a bad id in the third micro-batch of 2 documents"""
    r, m, _, q, d = _make(ROWS["d150_mask"])
    m._engine.docs_per_microbatch = 2
    b = _batch(q, d)
    with torch.no_grad():
        want = r.test(b)
        bad = dict(b, **{side: b[side].clone()})
        bad[side][pos] = value
        with pytest.raises(IndexError, match=("query" if side == "query" else "document") + " term id"):
            r.test(bad)
        again = r.test(b)
    assert torch.isfinite(again).all()
    assert torch.equal(again, want)
