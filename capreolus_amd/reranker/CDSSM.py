"""CDSSM (Shen et al., CIKM'14), behind the reference plugin surface (capreolus/reranker/CDSSM.py).

The module tree carries the reference's state_dict names (``embedding.weight``, ``conv.0.weight``, ``conv.0.bias``, ``ffw.weight``,
``ffw.bias``), so checkpoints interchange in both directions.  Scoring (`test`, eval-mode forward) runs the tower kernel once per side
(capamd_cdssm_tower, csrc/dssm.hip) and the pair kernel (capamd_cos_sigmoid_pairs) in fp32; `score` in training mode runs the
restatement below under autograd.

Semantics (reference CDSSM.py), quirks included:
  - x = embedding(ids): the frozen table's row 0 is read as the table has it, nothing masks pads;
  - W - T % W zero rows are appended - never none: a length that is a multiple of W gets a whole window of zeros - and the rows are cut
    into windows of W dim floats;
  - Conv1d(1, nfilter, nkernel) + ReLU over each FLATTENED window (a tap sequence runs across word boundaries inside a window), the
    per-window outputs concatenated on the channel axis and max(dim=1) over them: ONE max over windows and filters,
    rep[t] = max_i max_f relu(b_f + sum_j w[f][j] x_i[t + j]), W dim - nkernel + 1 values;
  - rep / (|rep| + 1e-7) per side, the dot product, the sigmoid: an all-zero representation on either side scores exactly 0.5;
  - `ffw` = Linear(nkernel, nhiddens) is in the state_dict and never used; dropout (after the ReLU) is live in training mode only.
Neither side ever sees the other before the cosine, so `test_pairs` runs the tower once per distinct row and scores (query row, document
row) pairs from the outputs.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import engine
from . import Reranker

# the limits of capamd_cdssm_tower (include/capreolus_amd.h)
MAX_DIM, MAX_WINDOW, MAX_SPAN, MAX_KERNEL, MAX_FILTER = 512, 8, 4096, 16, 16


class CDSSM_class(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.p = config
        weights = torch.as_tensor(np.asarray(extractor.embeddings, dtype=np.float32))
        self.embedding = nn.Embedding(*weights.shape)
        self.embedding.weight.data.copy_(weights)
        self.embedding.weight.requires_grad = False
        self.conv = nn.Sequential(nn.Conv1d(1, config["nfilter"], config["nkernel"]), nn.ReLU(), nn.Dropout(config["dropoutrate"]))
        self.ffw = nn.Linear(config["nkernel"], config["nhiddens"])     # (in the reference's state_dict, never used in its forward)
        self._engine = engine.CdssmEngine()

    def _params(self):
        return dict(self.named_parameters())

    def forward(self, sentence, query):
        """[B] scores of document ids [B, L] against query ids [B, Q] (the reference's argument order)"""
        if torch.is_grad_enabled() and self.training:
            return self._forward_aten(sentence, query)
        return self.forward_engine(sentence, query)

    def forward_engine(self, doctoks, querytoks, pair_q=None, pair_d=None, towers=False):
        """fp32 scores (and both tower outputs with towers=True) through the kernels; pair i is row i of both sides, or the index arrays'"""
        return self._engine.forward(querytoks, doctoks, self._params(), self.p["windowsize"], pair_q=pair_q, pair_d=pair_d, towers=towers)

    # ---- the restatement under autograd (training; also what the tests hold against the reference's fixtures, and in float64) ----

    def _tower_aten(self, toks, dtype):
        W = self.p["windowsize"]
        x = self.embedding(toks).to(dtype)                                   # [B, T, H]
        B, T, H = x.shape
        x = torch.cat([x, x.new_zeros(B, W - T % W, H)], dim=1).reshape(-1, 1, W * H)     # [B K, 1, W H]
        y = F.relu(F.conv1d(x, self.conv[0].weight.to(dtype), self.conv[0].bias.to(dtype)))
        y = self.conv[2](y)                                                  # dropout: identity outside training mode
        return y.reshape(B, -1, y.shape[-1]).max(dim=1)[0]                   # windows x filters on one axis, one max over it

    def _forward_aten(self, doctoks, querytoks, dtype=torch.float32, return_towers=False):
        q, d = self._tower_aten(querytoks, dtype), self._tower_aten(doctoks, dtype)
        cos = ((q / (q.norm(dim=-1)[:, None] + 1e-7)) * (d / (d.norm(dim=-1)[:, None] + 1e-7))).sum(dim=-1)
        score = torch.sigmoid(cos)
        return (score, q, d) if return_towers else score


class CDSSM(Reranker):
    """Yelong Shen, Xiaodong He, Jianfeng Gao, Li Deng, and Grégoire Mesnil. 2014. A Latent Semantic Model with Convolutional-Pooling
    Structure for Information Retrieval. In CIKM'14.  (reference capreolus/reranker/CDSSM.py)"""

    module_name = "CDSSM"
    supports_resident = True   # term-id rows: served from a device-resident CandidateStore (Reranker.test_resident)
    supports_lists = False
    config_spec = {"nkernel": 3, "nfilter": 1, "nhiddens": 30, "windowsize": 3, "dropoutrate": 0}

    def build_model(self):
        if not hasattr(self, "model"):
            c = self.config
            D = np.asarray(self.extractor.embeddings).shape[1]
            W, nk, nf = int(c["windowsize"]), int(c["nkernel"]), int(c["nfilter"])
            if not 1 <= D <= MAX_DIM or not 1 <= W <= MAX_WINDOW or W * D > MAX_SPAN:
                raise ValueError(f"CDSSM takes embeddings of dim 1..{MAX_DIM}, windowsize 1..{MAX_WINDOW} and windowsize x dim <= {MAX_SPAN}; "
                                 f"got dim {D}, windowsize {W}")
            if not 1 <= nk <= min(MAX_KERNEL, W * D):
                raise ValueError(f"CDSSM takes nkernel 1..min({MAX_KERNEL}, windowsize x dim = {W * D}); got nkernel {nk}")
            if not 1 <= nf <= MAX_FILTER:
                raise ValueError(f"CDSSM takes nfilter 1..{MAX_FILTER}; got nfilter {nf}")
            self.model = CDSSM_class(self.extractor, self.config)
        return self.model

    def score(self, d):
        return [self.model(d["posdoc"], d["query"]).view(-1), self.model(d["negdoc"], d["query"]).view(-1)]

    def test(self, d):
        return self.model(d["posdoc"], d["query"]).view(-1)

    def test_pairs(self, q, docs, pair_q, pair_d):
        """query ids [Nq, Q] and document ids [Nd, L], each row through the tower ONCE, then the (pair_q[i], pair_d[i]) pairs: one query
        against its candidates is q of one row and pair_q of zeros.  Bit-identical to `test` on the gathered rows."""
        return self.model.forward_engine(docs, q, pair_q=pair_q, pair_d=pair_d)

    def zero_grad(self, *args, **kwargs):
        self.model.zero_grad(*args, **kwargs)
