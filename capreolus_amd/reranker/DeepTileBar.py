"""DeepTileBar (Tang & Yang, AAAI'19), behind the reference plugin surface (capreolus/reranker/DeepTileBar.py).

The module tree carries the reference's state_dict names (``DeepTileBar1.conv{1..10}.{weight,bias}``,
``DeepTileBar1.lstm{1..10}.{weight_ih_l0,weight_hh_l0,bias_ih_l0,bias_hh_l0}``, ``DeepTileBar1.W{1,2,3}.{weight,bias}``), so checkpoints
interchange in both directions.  Scoring (`test`, eval-mode forward) is one C-ABI call (capamd_deeptile_forward, csrc/deeptile.hip) in
fp32; `score` in training mode runs the restatement below under autograd.  `test_ids` also colours the tiles on the device
(capamd_deeptile_color) from term ids and segment boundaries.  DeepTileBar is exported from this package and is not in `registry`.
Text tiling itself (nltk.TextTilingTokenizer) stays with the caller: the engine takes its boundaries.

Semantics of the model (reference DeepTileBar.py), per document:
  - the tile [Q, P, C] is seen as [C, Q, P]; Q and C come from the extractor's config (`maxqlen`; `tfchannel` false drops the tf channel,
    C = 2), P from the tensor;
  - conv_w, w = 1 .. 10, has a kernel of (Q, w): the whole query axis is consumed; `numberfilter` filters plus bias, no activation; its
    output is a sequence of T_w = P - w + 1 steps;
  - lstm_w (gates i, f, g, o, both biases, zero initial state: the reference resets its hidden state before every call) runs over that
    sequence and only the last h is kept; the ten h are concatenated in order 1 .. 10;
  - relu(W1 .), relu(W2 .), W3.
Semantics of the colouring (reference deeptileextractor.py, color_grid), per (query term q, segment):
  - a pad query term (id 0) or a pad segment (an empty range, see capreolus_amd/deeptiles.py) gives an all-zero tile;
  - tf = the segment's tokens whose id equals q; channels [tf, idf if tf else 0, sim], without tf when C = 2;
  - sim = max over the segment's tokens of exp(-|emb[t] - emb[q]|^2 / 2); the literal pad token (id -1) contributes 0, a word the
    vocabulary does not know (id 0) is looked up as the zero row like any other.
Two facts of the reference, noted and kept: the extractor's `passagelen` overrides the reranker's (the model's config is updated with the
extractor's), and `clean_segments` pads or collapses to 30 segments whatever `passagelen` says, so only the first P are coloured.

Differences from the reference:
  - `numberfilter` != 3 cannot run there (it hard-codes nn.LSTM(input_size=3)), nor can P < 10 (conv10 needs ten columns): both are
    refused with ValueError, as are the kernel's limits (P <= 64, maxqlen <= 32, lstmhiddendim <= 16, linear widths <= 128);
  - the reference only takes batches of exactly trainer.config["batch"] documents.  Documents are independent in the model, so any batch
    size is taken here and no trainer is needed.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import engine
from . import Reranker

WIDTHS = tuple(range(1, 11))
# the limits of capamd_deeptile_forward (include/capreolus_amd.h)
FILTERS, MIN_SEGMENTS, MAX_SEGMENTS, MAX_QLEN, MAX_HIDDEN, MAX_LINEAR = 3, 10, 64, 32, 16, 128


class DeepTileBar_nn(nn.Module):
    def __init__(self, maxqlen, channels, number_filter, lstm_hidden_dim, linear_hidden_dim1, linear_hidden_dim2):
        super().__init__()
        self.maxqlen, self.tilechannels = maxqlen, channels
        for w in WIDTHS:
            setattr(self, f"conv{w}", nn.Conv2d(channels, number_filter, (maxqlen, w), stride=1))
        for w in WIDTHS:
            setattr(self, f"lstm{w}", nn.LSTM(input_size=3, hidden_size=lstm_hidden_dim))
        self.W1 = nn.Linear(10 * lstm_hidden_dim, linear_hidden_dim1, bias=True)
        self.W2 = nn.Linear(linear_hidden_dim1, linear_hidden_dim2, bias=True)
        self.W3 = nn.Linear(linear_hidden_dim2, 1, bias=True)


def _lstm_last(lstm, seq):
    """nn.LSTM (one layer, gates i, f, g, o) over seq [T, B, 3] from zero state -> the last h [B, H], in seq's dtype"""
    w_ih, w_hh, b_ih, b_hh = (getattr(lstm, n + "_l0").to(seq.dtype) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    h = c = seq.new_zeros(seq.shape[1], w_hh.shape[1])
    for t in range(seq.shape[0]):
        i, f, g, o = (F.linear(seq[t], w_ih, b_ih) + F.linear(h, w_hh, b_hh)).chunk(4, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
    return h


def as_tiles(x):
    """the reference's `torch.cat([d["posdoc"][i] for i in range(len(d["qid"]))])`: a batch of [1, Q, P, C] tiles -> [B, Q, P, C]"""
    x = torch.as_tensor(x)
    if x.dim() == 5 and x.shape[1] == 1:
        return x.reshape(x.shape[0], *x.shape[2:])
    if x.dim() != 4:
        raise ValueError(f"DeepTileBar takes a batch of [1, Q, P, C] tiles (or [B, Q, P, C]); got {tuple(x.shape)}")
    return x


class DeepTileBar_class(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.p = dict(config)
        self.p.update(dict(getattr(extractor, "config", None) or {}))       # (the extractor's passagelen overrides the reranker's)
        channels = 3 if self.p.get("tfchannel", True) else 2
        self.DeepTileBar1 = DeepTileBar_nn(int(self.p["maxqlen"]), channels, int(config["numberfilter"]), int(config["lstmhiddendim"]),
                                           int(config["linearhiddendim1"]), int(config["linearhiddendim2"]))
        self._engine = engine.DeepTileEngine()

    def _params(self):
        return dict(self.named_parameters())

    def _check(self, tiles):
        m = self.DeepTileBar1
        B, Q, P, C = tiles.shape
        if Q != m.maxqlen or C != m.tilechannels or not MIN_SEGMENTS <= P <= MAX_SEGMENTS:
            raise ValueError(f"DeepTileBar takes tiles [B, {m.maxqlen}, P, {m.tilechannels}] with {MIN_SEGMENTS} <= P <= {MAX_SEGMENTS} (conv10 needs "
                             f"ten columns); got {tuple(tiles.shape)}")
        return P

    def test_forward(self, pos_tile_matrix):
        """[B] scores of tiles [B, Q, P, C]"""
        tiles = as_tiles(pos_tile_matrix)
        if torch.is_grad_enabled() and self.training:
            return self._forward_aten(tiles)
        return self.forward_engine(tiles)

    def forward(self, pos_tile_matrix, neg_tile_matrix):
        return [self.test_forward(pos_tile_matrix), self.test_forward(neg_tile_matrix)]

    def forward_engine(self, tiles, evidence=False):
        """capamd_deeptile_forward: fp32 scores [B] (and the [B, 10, H] last hidden states, the input of W1, with evidence=True)"""
        tiles = as_tiles(tiles)
        self._check(tiles)
        return self._engine.forward(tiles, self._params(), evidence=evidence)

    # ---- the restatement under autograd (training; also what the tests hold against the reference's fixtures, and in float64) ----

    def _forward_aten(self, tiles, dtype=torch.float32, return_evidence=False):
        m = self.DeepTileBar1
        tiles = as_tiles(tiles)
        self._check(tiles)
        B = tiles.shape[0]
        x = tiles.to(dtype).permute(0, 3, 1, 2)                                         # [B, C, Q, P]
        hs = []
        for w in WIDTHS:
            conv = getattr(m, f"conv{w}")
            seq = F.conv2d(x, conv.weight.to(dtype), conv.bias.to(dtype)).view(B, conv.weight.shape[0], -1).permute(2, 0, 1)     # [T_w, B, 3]
            hs.append(_lstm_last(getattr(m, f"lstm{w}"), seq))
        ev = torch.cat(hs, dim=1)                                                        # [B, 10 H]
        x1 = F.relu(F.linear(ev, m.W1.weight.to(dtype), m.W1.bias.to(dtype)))
        x2 = F.relu(F.linear(x1, m.W2.weight.to(dtype), m.W2.bias.to(dtype)))
        score = F.linear(x2, m.W3.weight.to(dtype), m.W3.bias.to(dtype)).view(-1)
        return (score, ev.view(B, 10, -1)) if return_evidence else score


class DeepTileBar(Reranker):
    """Zhiwen Tang and Grace Hui Yang. 2019. DeepTileBars: Visualizing Term Distribution for Neural Information Retrieval. In AAAI'19.
    (reference capreolus/reranker/DeepTileBar.py)"""

    module_name = "DeepTileBar"
    supports_resident = False   # the candidate store holds id rows without segment boundaries
    supports_lists = False
    config_spec = {"passagelen": 30, "numberfilter": 3, "lstmhiddendim": 3, "linearhiddendim1": 32, "linearhiddendim2": 16}

    def build_model(self):
        if not hasattr(self, "model"):
            c = self.config
            ex = dict(getattr(self.extractor, "config", None) or {})
            if "maxqlen" not in ex:
                raise ValueError("DeepTileBar reads maxqlen (and tfchannel, passagelen) from extractor.config")
            if int(c["numberfilter"]) != FILTERS:
                raise ValueError(f"DeepTileBar runs with numberfilter = 3 only (the reference hard-codes nn.LSTM(input_size=3)); got {c['numberfilter']}")
            P = int(ex.get("passagelen", c["passagelen"]))
            if not MIN_SEGMENTS <= P <= MAX_SEGMENTS or not 1 <= int(ex["maxqlen"]) <= MAX_QLEN:
                raise ValueError(f"DeepTileBar takes {MIN_SEGMENTS} <= passagelen <= {MAX_SEGMENTS} (conv10 needs ten columns) and maxqlen <= {MAX_QLEN}; "
                                 f"got passagelen {P}, maxqlen {ex['maxqlen']}")
            if ex.get("tilechannels", 3) not in (2, 3):
                raise ValueError(f"DeepTileBar tiles have 2 or 3 channels; got tilechannels {ex['tilechannels']}")
            if not (1 <= int(c["lstmhiddendim"]) <= MAX_HIDDEN and 1 <= int(c["linearhiddendim1"]) <= MAX_LINEAR and 1 <= int(c["linearhiddendim2"]) <= MAX_LINEAR):
                raise ValueError(f"DeepTileBar takes lstmhiddendim <= {MAX_HIDDEN} and linear widths <= {MAX_LINEAR}; got {c['lstmhiddendim']}, "
                                 f"{c['linearhiddendim1']}, {c['linearhiddendim2']}")
            self.model = DeepTileBar_class(self.extractor, c)
        return self.model

    def score(self, d):
        return self.model(d["posdoc"], d["negdoc"])

    def test(self, d):
        return self.model.test_forward(d["posdoc"])

    def _table(self, device):
        t = getattr(self, "_emb", None)
        if t is None or t.device != torch.device(device):
            t = self._emb = torch.as_tensor(np.asarray(self.extractor.embeddings, dtype=np.float32)).to(device)
        return t

    def color(self, d, emb=None):
        """the tiles [B, Q, P, C] of int64 `query` [B, Q] (pad 0), fp32 `query_idf` [B, Q], int64 `posdoc` ids [B, L] and int32
        `posdoc_segments` offsets [B, P + 1] (capreolus_amd.deeptiles.encode_segments), coloured on the device; emb: the fp32 table on
        the device (None: extractor.embeddings, moved there once)"""
        q = d["query"]
        emb = self._table(q.device) if emb is None else emb
        return self.model._engine.color(q, d["posdoc"], d["posdoc_segments"], d["query_idf"], emb, self.model.DeepTileBar1.tilechannels)

    def test_ids(self, d, emb=None):
        """colours and scores on the device; equals `test` on the coloured tiles bit for bit"""
        return self.model.test_forward(self.color(d, emb))
