"""HINT (Fan et al., SIGIR'18), behind the reference plugin surface (capreolus/reranker/HINT.py).

The module tree carries the reference's state_dict names (``HiNT1.embedding.weight``, ``HiNT1.Ws``, ``HiNT1.GRU2d1.gru_cell.{Wrz,W,U}``,
``HiNT1.GRU2d3.gru_cell.*``, ``HiNT1.lstm.*``, ``HiNT1.Wv``, ``HiNT1.fc``; there is no GRU2d2), so checkpoints interchange in both
directions.  Scoring (`test`, eval-mode forward) is one C-ABI call (capamd_hint_forward, csrc/hint.hip) in fp32; `score` in training
mode runs the restatement below under autograd.

Semantics (reference HINT.py), quirks included:
  - cos = (q / (|q| + 1e-7)) . (d / (|d| + 1e-7)): each side normalised on its own;
  - xor is 1 where the ids are equal, pad against pad included;
  - channels [Ws(emb[q_i]), Ws(emb[d_j]), M_ij] (bias included), all three multiplied by 1 - mask, where the mask is true only where
    BOTH ids are 0 (the reference hard-codes `== 0`; extractor.pad is not consulted);
  - windows of a hard-coded 100 terms: P = L // 100, the terms behind P x 100 are ignored;
  - GRUModel2d walks the query rows outside and the 100 columns inside from zero neighbours and returns the last row's last column;
    gru_cell(x, diag, top, left) builds q = [top, left, diag, x], `rl` gates top and `rt` gates left,
    h = zl left + zt top + zd diag + zi tanh(W x + U(r * [top, left, diag])), the four z softmaxed per hidden unit;
  - GRU2d1 runs on the xor and the cos tensor, GRU2d3 on both with the query and the column axis reversed; per window the 8-vector is
    [H_xor, H_cos, H_xor_inv, H_cos_inv];
  - the bidirectional LSTM runs over the P windows from zero state, its halves are ADDED; vt = tanh(Wv .); the 2P rows [vt; lstm] are
    top-kmax sorted per hidden unit and flattened unit x kmax + rank; fc gives the score.
`query_idf` is accepted and unused, as in the reference.

Two differences from the reference:
  - `spatialGRU` != 2, `LSTMdim` != 6 and kmax > 2P cannot run there (it hard-codes view(-1, 1, 2) and [:, :, :6]; topk fails): they are
    refused with ValueError, at build_model or at the call;
  - the reference only takes batches of exactly trainer.config["batch"] pairs.  Documents are independent in the model, so any batch
    size is taken here; Q, L and P come from the tensors and no trainer is needed.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import engine
from . import Reranker

WINDOW = 100
# the limits of capamd_hint_forward (include/capreolus_amd.h)
MAX_DIM, MAX_QLEN, MAX_WINDOWS, MAX_KMAX = 512, 32, 64, 32


class GRUCell2d(nn.Module):
    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.Wrz = nn.Linear(3 * hidden_size + input_size, 7 * hidden_size)
        self.W = nn.Linear(input_size, hidden_size)
        self.U = nn.Linear(3 * hidden_size, hidden_size)


class GRUModel2d(nn.Module):
    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        self.gru_cell = GRUCell2d(input_dim, hidden_dim)


class HiNT(nn.Module):
    def __init__(self, weights_matrix, p):
        super().__init__()
        weights = torch.as_tensor(np.asarray(weights_matrix, dtype=np.float32))
        self.embedding = nn.Embedding(*weights.shape)
        self.embedding.weight.data.copy_(weights)
        self.embedding.weight.requires_grad = False
        self.Ws = nn.Linear(weights.shape[1], 1)
        self.GRU2d1 = GRUModel2d(3, p["spatialGRU"])
        self.GRU2d3 = GRUModel2d(3, p["spatialGRU"])
        self.lstm = nn.LSTM(input_size=4 * p["spatialGRU"], hidden_size=p["LSTMdim"], bidirectional=True)
        self.Wv = nn.Linear(4 * p["spatialGRU"], p["LSTMdim"])
        self.fc = nn.Linear(p["LSTMdim"] * p["kmax"], 1)


def _spatial_gru(cells, S):
    """S [2, N, Q, 100, 3] (GRU2d1's input, GRU2d3's already reversed) -> the last cell's state [2, N, 2]: both cells at once, as batched
    products over the leading axis"""
    Wrz, bWrz = torch.stack([c.Wrz.weight for c in cells]).transpose(1, 2).to(S.dtype), torch.stack([c.Wrz.bias for c in cells]).unsqueeze(1).to(S.dtype)
    W, bW = torch.stack([c.W.weight for c in cells]).transpose(1, 2).to(S.dtype), torch.stack([c.W.bias for c in cells]).unsqueeze(1).to(S.dtype)
    U, bU = torch.stack([c.U.weight for c in cells]).transpose(1, 2).to(S.dtype), torch.stack([c.U.bias for c in cells]).unsqueeze(1).to(S.dtype)
    _, N, Q, T, _ = S.shape
    zero = S.new_zeros(2, N, 2)
    last = [zero] * (T + 1)
    for i in range(Q):
        row = [zero]
        for j in range(1, T + 1):
            x, diag, top, left = S[:, :, i, j - 1], last[j - 1], last[j], row[j - 1]
            t11 = torch.cat([top, left, diag], dim=-1)
            rz = torch.baddbmm(bWrz, torch.cat([t11, x], dim=-1), Wrz)             # [2, N, 14]
            r = torch.sigmoid(rz[..., :6])
            z = F.softmax(rz[..., 6:].reshape(2, N, 4, 2), dim=2)                  # zi, zl, zt, zd per hidden unit
            h1 = torch.tanh(torch.baddbmm(bW, x, W) + torch.baddbmm(bU, r * t11, U))
            row.append(z[:, :, 1] * left + z[:, :, 2] * top + z[:, :, 3] * diag + z[:, :, 0] * h1)
        last = row
    return last[-1]


def _lstm_direction(lstm, seq, suffix):
    """one direction of nn.LSTM (gates i, f, g, o) over seq [P, B, 8] from zero state -> [P, B, 6], in seq's dtype"""
    w_ih, w_hh, b_ih, b_hh = (getattr(lstm, n + "_l0" + suffix).to(seq.dtype) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
    h = c = seq.new_zeros(seq.shape[1], w_hh.shape[1])
    out = [None] * seq.shape[0]
    for t in (reversed(range(len(out))) if suffix else range(len(out))):
        i, f, g, o = (F.linear(seq[t], w_ih, b_ih) + F.linear(h, w_hh, b_hh)).chunk(4, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[t] = h
    return torch.stack(out)


class HiNT_main(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.p = config
        self.HiNT1 = HiNT(extractor.embeddings, config)
        self._engine = engine.HintEngine()

    def _params(self):
        return dict(self.named_parameters())

    def _check(self, doctoks, querytoks):
        P = doctoks.shape[1] // WINDOW
        if P < 1 or self.p["kmax"] > 2 * P:
            raise ValueError(f"HINT takes documents of at least {WINDOW} terms and kmax <= 2 P (P = L // {WINDOW} windows); got L "
                             f"{doctoks.shape[1]}, kmax {self.p['kmax']}")
        return P

    def test_forward(self, query_sentence, query_idf, pos_sentence):
        """[B] scores.  query_idf is accepted and ignored, as in the reference."""
        if torch.is_grad_enabled() and self.training:
            return self._forward_aten(pos_sentence, query_sentence)
        return self.forward_engine(pos_sentence, query_sentence)

    def forward(self, query_sentence, query_idf, pos_sentence, neg_sentence):
        return [self.test_forward(query_sentence, query_idf, pos_sentence), self.test_forward(query_sentence, query_idf, neg_sentence)]

    def forward_engine(self, doctoks, querytoks, evidence=False):
        """capamd_hint_forward: fp32 scores [B] (and the [B, P, 8] window evidence, the LSTM's input, with evidence=True)"""
        self._check(doctoks, querytoks)
        return self._engine.forward(querytoks, doctoks, self._params(), self.p["kmax"], evidence=evidence)

    # ---- the restatement under autograd (training; also what the tests hold against the reference's fixtures, and in float64) ----

    def _forward_aten(self, doctoks, querytoks, dtype=torch.float32, return_evidence=False):
        m = self.HiNT1
        P = self._check(doctoks, querytoks)
        B, Q = querytoks.shape
        T = P * WINDOW
        x, qx = m.embedding(doctoks).to(dtype), m.embedding(querytoks).to(dtype)
        cos = torch.matmul(qx / (qx.norm(dim=2)[:, :, None] + 1e-7), (x / (x.norm(dim=2)[:, :, None] + 1e-7)).transpose(1, 2))   # [B, Q, L]
        xor = (querytoks[:, :, None] == doctoks[:, None, :]).to(dtype)
        keep = 1 - ((querytoks == 0)[:, :, None] & (doctoks == 0)[:, None, :]).to(dtype)
        Xi = F.linear(qx, m.Ws.weight.to(dtype), m.Ws.bias.to(dtype))[:, :, 0]      # [B, Q]
        Yj = F.linear(x, m.Ws.weight.to(dtype), m.Ws.bias.to(dtype))[:, :, 0]       # [B, L]

        def windows(M):                                                            # [B, Q, L] -> [B P, Q, 100, 3], masked
            S = torch.stack([Xi[:, :, None].expand(B, Q, T), Yj[:, None, :T].expand(B, Q, T), M[:, :, :T]], dim=-1) * keep[:, :, :T, None]
            return S.view(B, Q, P, WINDOW, 3).permute(0, 2, 1, 3, 4).reshape(B * P, Q, WINDOW, 3)

        S = torch.cat([windows(xor), windows(cos)], dim=0)                         # [2 B P, Q, 100, 3]
        H = _spatial_gru([m.GRU2d1.gru_cell, m.GRU2d3.gru_cell], torch.stack([S, S.flip(1, 2)]))     # [2, 2 B P, 2]
        n = B * P
        ev = torch.cat([H[0, :n], H[0, n:], H[1, :n], H[1, n:]], dim=-1).view(B, P, 8)
        seq = ev.transpose(0, 1)                                                    # [P, B, 8]
        lstm_out = _lstm_direction(m.lstm, seq, "") + _lstm_direction(m.lstm, seq, "_reverse")     # the two halves are added
        vt = torch.tanh(F.linear(seq, m.Wv.weight.to(dtype), m.Wv.bias.to(dtype)))
        top, _ = torch.topk(torch.cat([vt, lstm_out], 0).transpose(0, 2), self.p["kmax"], largest=True, sorted=True, dim=2)   # [6, B, kmax]
        score = F.linear(top.transpose(0, 1).reshape(B, -1), m.fc.weight.to(dtype), m.fc.bias.to(dtype)).view(-1)
        return (score, ev) if return_evidence else score


class HINT(Reranker):
    """Yixing Fan, Jiafeng Guo, Yanyan Lan, Jun Xu, Chengxiang Zhai, and Xueqi Cheng. 2018. Modeling Diverse Relevance Patterns in Ad-hoc
    Retrieval. In SIGIR'18.  (reference capreolus/reranker/HINT.py)"""

    module_name = "HINT"
    supports_resident = True   # term-id rows: served from a device-resident CandidateStore (Reranker.test_resident)
    supports_lists = False
    config_spec = {"spatialGRU": 2, "LSTMdim": 6, "kmax": 10}

    def build_model(self):
        if not hasattr(self, "model"):
            c = self.config
            D = np.asarray(self.extractor.embeddings).shape[1]
            if int(c["spatialGRU"]) != 2 or int(c["LSTMdim"]) != 6:
                raise ValueError(f"HINT runs with spatialGRU = 2 and LSTMdim = 6 only (the reference hard-codes both widths in its forward); "
                                 f"got spatialGRU {c['spatialGRU']}, LSTMdim {c['LSTMdim']}")
            if not 1 <= int(c["kmax"]) <= MAX_KMAX or D > MAX_DIM:
                raise ValueError(f"HINT takes kmax 1..{MAX_KMAX} and embeddings of dim <= {MAX_DIM}; got kmax {c['kmax']}, dim {D}")
            maxdoclen = (getattr(self.extractor, "config", None) or {}).get("maxdoclen")
            if maxdoclen is not None and int(c["kmax"]) > 2 * (int(maxdoclen) // WINDOW):
                raise ValueError(f"HINT: kmax {c['kmax']} exceeds the 2 P = {2 * (int(maxdoclen) // WINDOW)} rows of evidence that documents of "
                                 f"maxdoclen {maxdoclen} give (P = maxdoclen // {WINDOW})")
            self.model = HiNT_main(self.extractor, self.config)
        return self.model

    def score(self, d):
        return self.model(d["query"], d["query_idf"], d["posdoc"], d["negdoc"])

    def test(self, d):
        return self.model.test_forward(d["query"], d["query_idf"], d["posdoc"])
