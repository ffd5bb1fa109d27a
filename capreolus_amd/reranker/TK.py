"""TK, the Transformer-Kernel reranker (Hofstätter et al., TREC'19), behind the reference plugin surface (capreolus/reranker/TK.py).

The module holds its parameters under the reference's state_dict names (``embedding.weight``, ``position_encoder.pe``, ``mixer``,
``transformer_encoder.layers.N.*``, ``{s_log,s_len,comb}_fcc.weight``), so checkpoints interchange in both directions.  Scoring
(`test`, eval-mode forward) is one C-ABI call (capamd_tk_forward, csrc/tk.hip) in fp32; `score` in training mode runs the restatement
below under autograd.

Semantics (reference TK.py :86-143), including its quirks:
  - x = emb[tok] + pe[:L] (dropout 0.1 on the sum in training mode); the encoder layers have dropout 0;
  - `usemask`: a position whose EMBEDDING ROW is all zeros (not id == pad) is excluded as query and key of its own sequence's attention,
    and a row that attends to nothing gets a zero attention output (then the out_proj bias).  The reference tiles its [B, L, L] mask
    head-major for nn.MultiheadAttention, whose rows are batch-major, so with several documents of different masks in one batch its
    head h of document b uses the mask of document (b * heads + h) mod B; here every document uses its own mask - the reference's
    result at batch size 1, and independent of what else is in the batch;
  - the mix a * emb + (1 - a) * ctx uses the raw embedding (without pe);
  - the kernel value is exp(-(c - mu)^2) / (2 sigma^2): the division comes after exp;
  - the kernel sums run over all L positions (pads too) and s_log sums log2 over all query rows; no biases, no tanh.
`scoretanh`, `singlefc`, `projdim`, `gradkernels` and `query_idf` are accepted and have no effect, as in the reference.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import engine
from . import Reranker

MUS = (-0.9, -0.7, -0.5, -0.3, -0.1, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0)
SIGMA = 0.1


class PositionalEncoding(nn.Module):
    """The sinusoidal table as the reference builds it ([max_len, 1, d_model] buffer `pe`, saved in checkpoints) and its dropout."""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(position * div)
        pe[:, 1::2] = torch.cos(position * div)
        self.register_buffer("pe", pe.unsqueeze(1))


class TK_class(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.p = config
        self.pad = int(getattr(extractor, "pad", 0))
        weights = torch.as_tensor(np.asarray(extractor.embeddings, dtype=np.float32))
        self.embeddim = weights.shape[1]
        self.embedding = nn.Embedding(*weights.shape)
        self.embedding.weight.data.copy_(weights)
        self.embedding.weight.requires_grad = bool(config["finetune"])
        self.position_encoder = PositionalEncoding(self.embeddim)
        self.mixer = nn.Parameter(torch.full([1, 1, 1], 0.9, dtype=torch.float32))
        layer = nn.TransformerEncoderLayer(self.embeddim, config["numattheads"], config["ffdim"], 0)
        self.transformer_encoder = nn.TransformerEncoder(layer, config["numlayers"], enable_nested_tensor=False)
        K = len(MUS)
        self.s_log_fcc = nn.Linear(K, 1, bias=False)
        self.s_len_fcc = nn.Linear(K, 1, bias=False)
        self.comb_fcc = nn.Linear(2, 1, bias=False)
        for lin in (self.s_log_fcc, self.s_len_fcc, self.comb_fcc):
            nn.init.uniform_(lin.weight, -0.014, 0.014)
        self._engine = engine.TKEngine()

    def _params(self):
        return dict(self.named_parameters(), **dict(self.named_buffers()))

    def forward(self, doctoks, querytoks, query_idf=None):
        """[B, 1] scores.  query_idf is accepted and ignored, as in the reference."""
        if torch.is_grad_enabled() and self.training:
            return self._forward_aten(doctoks, querytoks).view(-1, 1)
        return self.forward_engine(doctoks, querytoks).view(-1, 1)

    def forward_engine(self, doctoks, querytoks, features=False):
        """capamd_tk_forward: fp32 scores [B] (and the [B, 22] features s_log_k | s_len_k with features=True)"""
        layer = self.transformer_encoder.layers[0]
        return self._engine.forward(querytoks, doctoks, self._params(), layer.self_attn.num_heads, len(self.transformer_encoder.layers),
                                    self.p["usemask"], self.p["alpha"], self.pad, layer.norm1.eps,
                                    mixer=self.mixer if self.p["usemixer"] else None, features=features)

    # ---- the restatement under autograd (training; also what the CPU tests hold against the reference's fixtures) ----

    def _encode(self, toks):
        emb = self.embedding(toks)                                          # [B, S, D]
        S = toks.shape[1]
        x = self.position_encoder.dropout(emb + self.position_encoder.pe[:S, 0].unsqueeze(0))
        valid = (emb != 0).any(dim=-1) if self.p["usemask"] else None       # [B, S]: the embedding row is not all zeros
        for layer in self.transformer_encoder.layers:
            x = _encoder_layer(layer, x, valid)
        a = self.mixer if self.p["usemixer"] else self.p["alpha"]
        return a * emb + (1 - a) * x

    def _forward_aten(self, doctoks, querytoks, return_features=False):
        doc, query = self._encode(doctoks), self._encode(querytoks)
        L = doctoks.shape[1]
        q_den = query.norm(p=2, dim=2).unsqueeze(2) + 1e-9
        d_den = doc.norm(p=2, dim=2).unsqueeze(1) + 1e-9
        sim = query.bmm(doc.transpose(1, 2)) / (q_den * d_den)             # [B, Q, L]
        zero = torch.zeros_like(sim)
        sim = torch.where((querytoks == self.pad).unsqueeze(2), zero, sim)
        sim = torch.where((doctoks == self.pad).unsqueeze(1), zero, sim)
        mu = torch.tensor(MUS, dtype=torch.float32, device=sim.device).view(1, -1, 1, 1)
        sigma = torch.tensor(SIGMA, dtype=torch.float32)
        k = torch.exp(-torch.pow(sim.unsqueeze(1) - mu, 2)) / (2 * torch.pow(sigma, 2)).to(sim.device)
        ksum = k.sum(3)                                                      # [B, 11, Q]
        s_log_k = torch.log2(ksum).sum(2)
        s_len_k = ksum.sum(2) / L
        score = self.comb_fcc(torch.cat([self.s_log_fcc(s_log_k), self.s_len_fcc(s_len_k)], dim=1)).view(-1)
        return (score, torch.cat([s_log_k, s_len_k], dim=1)) if return_features else score


def _encoder_layer(layer, x, valid):
    """nn.TransformerEncoderLayer (post-norm, ReLU, dropout 0) over x [B, S, D]; valid [B, S] or None (see the module docstring)."""
    sa = layer.self_attn
    B, S, D = x.shape
    H = sa.num_heads
    hd = D // H
    q, k, v = (t.reshape(B, S, H, hd).transpose(1, 2) for t in F.linear(x, sa.in_proj_weight, sa.in_proj_bias).split(D, dim=-1))
    scores = (q @ k.transpose(-1, -2)) / math.sqrt(hd)                     # [B, H, S, S]
    if valid is None:
        p = torch.softmax(scores, dim=-1)
    else:
        allowed = (valid.unsqueeze(2) & valid.unsqueeze(1)).unsqueeze(1)    # [B, 1, S, S]
        dead = ~allowed.any(dim=-1, keepdim=True)                           # rows that attend to nothing: output 0
        scores = scores.masked_fill(~allowed, float("-inf")).masked_fill(dead, 0.0)
        p = torch.softmax(scores, dim=-1) * (~dead)
    ctx = (p @ v).transpose(1, 2).reshape(B, S, D)
    x = layer.norm1(x + F.linear(ctx, sa.out_proj.weight, sa.out_proj.bias))
    return layer.norm2(x + layer.linear2(F.relu(layer.linear1(x))))


# the limits of capamd_tk_forward (include/capreolus_amd.h)
MAX_DIM, MAX_HEAD_DIM, MAX_FFDIM, MAX_QLEN = 512, 64, 512, 32


class TK(Reranker):
    """Sebastian Hofstätter, Markus Zlabinger, and Allan Hanbury. 2019. TU Wien @ TREC Deep Learning '19 -- Simple Contextualization for
    Re-ranking. In TREC '19.  (reference capreolus/reranker/TK.py)"""

    module_name = "TK"
    supports_resident = True   # term-id rows: served from a device-resident CandidateStore (Reranker.test_resident)
    supports_lists = False
    config_spec = {"gradkernels": True, "scoretanh": False, "singlefc": True, "projdim": 32, "ffdim": 100, "numlayers": 2, "numattheads": 10,
                   "alpha": 0.5, "usemask": False, "usemixer": False, "finetune": False}

    def build_model(self):
        if not hasattr(self, "model"):
            D = np.asarray(self.extractor.embeddings).shape[1]
            c = self.config
            heads, ff, layers = int(c["numattheads"]), int(c["ffdim"]), int(c["numlayers"])
            if heads < 1 or D % heads or D > MAX_DIM or D // heads > MAX_HEAD_DIM or not 1 <= ff <= MAX_FFDIM or layers < 1:
                raise ValueError(f"TK takes embeddings of dim <= {MAX_DIM} split into heads of width <= {MAX_HEAD_DIM}, ffdim 1..{MAX_FFDIM} "
                                 f"and numlayers >= 1; got dim {D}, numattheads {heads}, ffdim {ff}, numlayers {layers}")
            self.model = TK_class(self.extractor, self.config)
        return self.model

    def score(self, d):
        return [self.model(d["posdoc"], d["query"], d["query_idf"]).view(-1), self.model(d["negdoc"], d["query"], d["query_idf"]).view(-1)]

    def test(self, d):
        return self.model(d["posdoc"], d["query"], d["query_idf"]).view(-1)
