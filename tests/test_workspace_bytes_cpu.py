"""capamd_{tk,hint,posit,parade}_workspace_bytes are part of the C ABI: callers size their buffers by them, and the entries carve the
workspace by the same statement of the layout (csrc/workspace.h).  Buffer order, element counts and the 256-byte rounding decide the
figures pinned here; a change of any of them is a change of the ABI.  Host calls only."""
import ctypes

import pytest

from capreolus_amd import _lib


def _tk(dim, heads, ffdim, numlayers):
    m = _lib.TkModel()
    m.vocab, m.pad, m.dim, m.heads, m.ffdim, m.numlayers, m.max_len, m.alpha, m.ln_eps = 1000, 0, dim, heads, ffdim, numlayers, 5000, 0.5, 1e-5
    return m


def _hint(dim, kmax):
    m = _lib.HintModel()
    m.vocab, m.dim, m.kmax = 1000, dim, kmax
    return m


def _posit(dim):
    m = _lib.PositModel()
    m.vocab, m.pad, m.dim = 1000, 0, dim
    return m


def _parade(hidden, ffn):
    m = _lib.ParadeHeadModel()
    m.hidden, m.heads, m.ffn, m.ln_eps = hidden, hidden // 64, ffn, 1e-12
    return m


# (entry, model, the entry's three integers: (docs per micro-batch, Q, L), for PARADE (B, P)) -> bytes
PINNED = [
    ("tk", _tk(300, 10, 100, 2), (1, 4, 800), 6574848),
    ("tk", _tk(300, 10, 100, 2), (2, 4, 800), 13149440),
    ("tk", _tk(300, 10, 100, 2), (1000, 4, 800), 6574720000),
    ("tk", _tk(512, 8, 512, 1), (3, 32, 64), 2974464),
    ("hint", _hint(300, 10), (1, 4, 800), 23296),
    ("hint", _hint(300, 10), (2, 4, 800), 45568),
    ("hint", _hint(300, 10), (1000, 4, 800), 22672128),
    ("hint", _hint(512, 2), (1, 32, 100), 14848),
    ("posit", _posit(300), (1, 4, 800), 13355776),
    ("posit", _posit(300), (16, 4, 800), 213688576),
    ("posit", _posit(300), (17, 4, 800), 227044352),
    ("posit", _posit(300), (1000, 4, 800), 5696016128),
    ("posit", _posit(300), (1 << 15, 4, 800), 169534291968),
    ("posit", _posit(300), (1 << 16, 4, 800), 339068583936),
    ("posit", _posit(50), (1, 16, 5), 58880),
    ("parade", _parade(768, 3072), (4, 8), 1327104),
    ("parade", _parade(64, 64), (1, 1), 4608),
    ("parade", _parade(64, 64), (0, 1), 0),
    # one refusal each: Q beyond 32, a document shorter than one window, a document shorter than 5 terms, no passage
    ("tk", _tk(300, 10, 100, 2), (1, 33, 800), -1),
    ("hint", _hint(300, 10), (1, 4, 99), -1),
    ("posit", _posit(300), (1, 4, 4), -1),
    ("parade", _parade(768, 3072), (4, 0), -1),
]


def _bytes(entry, model, args):
    return getattr(_lib.load(), f"capamd_{entry}_workspace_bytes")(ctypes.byref(model), *args)


@pytest.mark.parametrize("row", PINNED, ids=lambda r: "-".join(map(str, (r[0], getattr(r[1], "dim", None) or r[1].hidden, *r[2]))))
def test_workspace_bytes_are_pinned(row):
    entry, model, args, want = row
    assert _bytes(entry, model, args) == want, (entry, args)

