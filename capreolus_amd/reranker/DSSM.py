"""DSSM (Huang et al., CIKM'13), behind the reference plugin surface (capreolus/reranker/DSSM.py).

The module tree carries the reference's state_dict names (``ffw.linear0.weight``, ``ffw.linear0.bias``, ``ffw.linear1.weight``, ...),
so checkpoints interchange in both directions.  Scoring (`test`, eval-mode forward) runs the tower kernel once per side
(capamd_dssm_tower, csrc/dssm.hip) and the pair kernel (capamd_cos_sigmoid_pairs) in fp32; `score` in training mode runs the
restatement below under autograd.

Semantics (reference DSSM.py):
  - `ffw` is a Sequential of linear%d / activate%d (ReLU) / dropout%d (0.5, live in training mode only), one triple per entry of
    `nhiddens` (a string such as "56" or "56 128"); its input width is len(extractor.stoi);
  - the same `ffw` runs over the query's and over the document's bag of words; rep / (|rep| + 1e-7) per side, the dot product, the
    sigmoid;
  - `query_idf` is accepted and unused.
The reference reads a dense [B, nvocab] count matrix.  The kernels read bags in CSR form (capreolus_amd.bags.Bags): `test` takes
either under the same keys - a dense tensor is converted by bags.from_dense - and both give the same bits.  Neither side ever sees the
other before the cosine, so `test_pairs` runs the tower once per distinct row and scores (query row, document row) pairs from the
outputs.
"""
import torch
import torch.nn.functional as F
from torch import nn

from .. import bags as bagslib
from .. import engine
from . import Reranker

# the limits of capamd_dssm_tower (include/capreolus_amd.h)
MAX_LAYERS, MAX_WIDTH, MAX_VOCAB = 4, 512, 2 ** 31 - 1


class DSSM_class(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.nvocab = len(extractor.stoi)
        nhiddens = [self.nvocab] + list(map(int, str(config["nhiddens"]).split()))
        self.ffw = nn.Sequential()
        for i in range(len(nhiddens) - 1):
            self.ffw.add_module("linear%d" % i, nn.Linear(nhiddens[i], nhiddens[i + 1]))
            self.ffw.add_module("activate%d" % i, nn.ReLU())
            self.ffw.add_module("dropout%i" % i, nn.Dropout(0.5))
        self._engine = engine.DssmEngine()

    def _linears(self):
        return [(m.weight, m.bias) for m in self.ffw if isinstance(m, nn.Linear)]

    def forward(self, sentence, query, query_idf=None):
        """[B] scores of document bags against query bags (the reference's argument order; query_idf is accepted and ignored)"""
        if torch.is_grad_enabled() and self.training:
            return self._forward_aten(sentence, query)
        return self.forward_engine(sentence, query)

    @staticmethod
    def _bags(x):
        return x if isinstance(x, bagslib.Bags) else bagslib.from_dense(x)

    def forward_engine(self, sentence, query, pair_q=None, pair_d=None, towers=False):
        """fp32 scores (and both tower outputs with towers=True) through the kernels, from Bags or from dense [N, nvocab] matrices; pair i
        is row i of both sides, or the index arrays'"""
        for x in (sentence, query):
            if not isinstance(x, bagslib.Bags) and (x.dim() != 2 or x.shape[1] != self.nvocab):
                raise ValueError(f"DSSM reads [N, {self.nvocab}] bag-of-words matrices (or Bags); got {tuple(x.shape)}")
        return self._engine.forward(self._bags(query), self._bags(sentence), self._linears(), pair_q=pair_q, pair_d=pair_d, towers=towers)

    # ---- the restatement under autograd (training; also what the tests hold against the reference's fixtures, and in float64) ----

    def _tower_aten(self, x, dtype):
        if isinstance(x, bagslib.Bags):
            x = x.to_dense(self.nvocab, dtype)
        x = x.to(dtype)
        for m in self.ffw:
            x = F.linear(x, m.weight.to(dtype), m.bias.to(dtype)) if isinstance(m, nn.Linear) else m(x)   # (dropout: identity outside training)
        return x

    def _forward_aten(self, sentence, query, dtype=torch.float32, return_towers=False):
        q, d = self._tower_aten(query, dtype), self._tower_aten(sentence, dtype)
        cos = ((q / (q.norm(dim=-1)[:, None] + 1e-7)) * (d / (d.norm(dim=-1)[:, None] + 1e-7))).sum(dim=-1)
        score = torch.sigmoid(cos)
        return (score, q, d) if return_towers else score


class DSSM(Reranker):
    """Po-Sen Huang, Xiaodong He, Jianfeng Gao, Li Deng, Alex Acero, and Larry Heck. 2013. Learning deep structured semantic models for
    web search using clickthrough data. In CIKM'13.  (reference capreolus/reranker/DSSM.py)"""

    module_name = "DSSM"
    supports_resident = False  # the candidate store holds padded id rows, and a pad is not a bag entry
    supports_lists = False
    config_spec = {"nhiddens": "56"}

    def build_model(self):
        if not hasattr(self, "model"):
            try:
                widths = list(map(int, str(self.config["nhiddens"]).split()))
            except ValueError:
                raise ValueError(f"DSSM: nhiddens is a string of layer widths such as '56' or '56 128'; got {self.config['nhiddens']!r}") from None
            nvocab = len(self.extractor.stoi)
            if not 1 <= len(widths) <= MAX_LAYERS:
                raise ValueError(f"DSSM takes 1..{MAX_LAYERS} layers; got nhiddens {self.config['nhiddens']!r}")
            if any(not 1 <= h <= MAX_WIDTH for h in widths):
                raise ValueError(f"DSSM takes hidden widths 1..{MAX_WIDTH}; got nhiddens {self.config['nhiddens']!r}")
            if not 1 <= nvocab <= MAX_VOCAB:
                raise ValueError(f"DSSM takes a vocabulary of 1..2^31 - 1 terms; got {nvocab}")
            self.model = DSSM_class(self.extractor, self.config)
        return self.model

    def score(self, d):
        return [self.model(d["posdoc"], d["query"], d.get("query_idf")).view(-1), self.model(d["negdoc"], d["query"], d.get("query_idf")).view(-1)]

    def test(self, d):
        return self.model(d["posdoc"], d["query"], d.get("query_idf")).view(-1)

    def test_pairs(self, q, docs, pair_q, pair_d):
        """query bags of Nq rows and document bags of Nd rows (Bags or dense), each row through the tower ONCE, then the
        (pair_q[i], pair_d[i]) pairs: one query against its candidates is q of one row and pair_q of zeros.  Bit-identical to `test` on
        the gathered rows."""
        return self.model.forward_engine(docs, q, pair_q=pair_q, pair_d=pair_d)
