"""DUET (Mitra, Diaz and Craswell, WWW'17), behind the reference plugin surface (capreolus/reranker/DUET.py).

The module tree carries the reference's state_dict names (``lm.conv.0``, ``lm.ffw.0``, ``lm.ffw.3``, ``dm.embedding``, ``dm.q_conv.0``,
``dm.q_ffw.0``, ``dm.d_conv1.0``, ``dm.d_conv2.0``, ``dm.ffw_1.0``, ``dm.ffw_2.1``), so a reference checkpoint loads with
``load_state_dict``.  Scoring (`test`, eval-mode forward) on a GPU is one C-ABI call (capamd_duet_forward, csrc/duet.hip) in fp32; `score`
in training mode, and everything on the CPU, runs the restatement below.

Semantics (reference DUET.py), quirks included; Q = maxqlen, L = maxdoclen, H = nfilters:
  - local model: lm[b, q, d] = (query[b, q] == doc[b, d]) (x idf[b, q] with `idfweight`).  Ids are compared without any mask: a pad in
    the query matches every pad in the document.  Conv2d(1, H, (1, L)) spans the whole document: x[b, h, q] = act(W[h] . lm[b, q] + b[h]);
    the feed-forward input is x flattened h Q + q; Linear, act, dropout, Linear;
  - distributed model, query: Conv2d(1, H, (3, dim)) over the Q - 2 windows of three embedding rows, act, dropout, MaxPool2d((2, 1),
    stride 1) - at Q = 4 the maximum of the two windows -, then q_ffw without an activation;
  - distributed model, document: the same convolution over the L - 2 windows, act, dropout, MaxPool2d((100, 1), stride 1): a sliding
    maximum of 100 over L - 2 positions, L - 101 values per filter; Conv2d(1, H, (H, 1)) mixes the filters per position, act, dropout;
    the product with the query vector; Linear(nhidden, 1) over the positions, act; dropout, Linear(H, 1) over the filters;
  - score = lm + dm.  The embedding table is read as it is: row 0 is not forced to zero.

The reference only runs in a narrow range: its bare `.squeeze()` calls and fixed pooling windows need maxqlen == 4, nfilters >= 2,
maxdoclen >= 103, nhidden == maxdoclen - 101, and a batch of at least 2.  The first four are refused here with a ValueError that names the
condition; a batch of one works: this restatement squeezes named axes only.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import engine
from . import Reranker

POOL = 100
# the limits of capamd_duet_forward (include/capreolus_amd.h)
QLEN, MIN_FILTERS, MAX_FILTERS, MAX_LMHIDDEN, MAX_DIM, MIN_DOCLEN, MAX_DOCLEN = 4, 2, 32, 256, 512, POOL + 3, 8192


def check_geometry(maxqlen, maxdoclen, nfilters, nhidden):
    """ValueError naming the first of the four conditions outside which the reference itself does not run"""
    if int(maxqlen) != QLEN:
        raise ValueError(f"DUET runs with maxqlen == {QLEN} only (the query convolution's two windows are pooled into one); got maxqlen {maxqlen}")
    if int(nfilters) < MIN_FILTERS:
        raise ValueError(f"DUET needs nfilters >= {MIN_FILTERS}; got nfilters {nfilters}")
    if int(maxdoclen) < MIN_DOCLEN:
        raise ValueError(f"DUET needs maxdoclen >= {MIN_DOCLEN} (a sliding maximum of {POOL} over maxdoclen - 2 positions, at least two of them "
                         f"left); got maxdoclen {maxdoclen}")
    if int(nhidden) != int(maxdoclen) - (POOL + 1):
        raise ValueError(f"DUET needs nhidden == maxdoclen - {POOL + 1} = {int(maxdoclen) - (POOL + 1)}; got nhidden {nhidden}")


def _activation(name):
    if name == "tanh":
        return nn.Tanh()
    if name == "relu":
        return nn.ReLU()
    raise ValueError("Unexpected activation: should be either tanh or relu")


class LocalModel(nn.Module):
    def __init__(self, p, q_len, doc_len):
        super().__init__()
        act = _activation(p["activation"])
        self.conv = nn.Sequential(nn.Conv2d(1, p["nfilters"], (1, doc_len)), act)
        self.ffw = nn.Sequential(nn.Linear(q_len * p["nfilters"], p["lmhidden"]), act, nn.Dropout(p["dropoutrate"]), nn.Linear(p["lmhidden"], 1))


class DistributedModel(nn.Module):
    def __init__(self, weights_matrix, p):
        super().__init__()
        act = _activation(p["activation"])
        weights = torch.as_tensor(np.asarray(weights_matrix, dtype=np.float32))
        self.embedding = nn.Embedding(*weights.shape)
        self.embedding.weight.data.copy_(weights)
        self.embedding.weight.requires_grad = False
        dim, H, rate = weights.shape[1], p["nfilters"], p["dropoutrate"]
        self.q_conv = nn.Sequential(nn.Conv2d(1, H, (3, dim)), act, nn.Dropout(rate), nn.MaxPool2d((2, 1), stride=(1, 1)))
        self.q_ffw = nn.Sequential(nn.Linear(H, H))
        self.d_conv1 = nn.Sequential(nn.Conv2d(1, H, (3, dim)), act, nn.Dropout(rate), nn.MaxPool2d((POOL, 1), stride=(1, 1)))
        self.d_conv2 = nn.Sequential(nn.Conv2d(1, H, (H, 1)), act, nn.Dropout(rate))
        self.ffw_1 = nn.Sequential(nn.Linear(p["nhidden"], 1), act)
        self.ffw_2 = nn.Sequential(nn.Dropout(rate), nn.Linear(H, 1))


class DUET_class(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.p = config
        ec = extractor.config
        check_geometry(ec["maxqlen"], ec["maxdoclen"], config["nfilters"], config["nhidden"])
        self.lm = LocalModel(config, ec["maxqlen"], ec["maxdoclen"])
        self.dm = DistributedModel(extractor.embeddings, config)
        self._engine = engine.DuetEngine(config["activation"], config["idfweight"])

    def _params(self):
        return dict(self.named_parameters())

    def _check(self, documents, queries):
        check_geometry(queries.shape[1], documents.shape[1], self.p["nfilters"], self.p["nhidden"])
        if documents.shape[1] != self.lm.conv[0].weight.shape[-1]:
            raise ValueError(f"DUET: documents of {documents.shape[1]} terms for a model of maxdoclen {self.lm.conv[0].weight.shape[-1]}")

    def forward(self, documents, queries, query_idf):
        """[B] scores of document ids [B, L] against query ids [B, Q] (the reference's argument order)"""
        if documents.is_cuda and not (torch.is_grad_enabled() and self.training):
            return self.forward_engine(documents, queries, query_idf)
        return self._forward_aten(documents, queries, query_idf)

    def forward_engine(self, documents, queries, query_idf, parts=False, evidence=False, check=True):
        """capamd_duet_forward: fp32 scores [B] (with parts=True also (lm, dm) [B, 2]; with evidence=True also the query vector [B, H] and
        the pooled map [B, H, L - 101])"""
        self._check(documents, queries)
        return self._engine.forward(queries, query_idf, documents, self._params(), parts=parts, evidence=evidence, check=check)

    # ---- the restatement under autograd (training, the CPU; also what the tests hold against the reference's fixtures) ----

    def _forward_aten(self, documents, queries, query_idf, dtype=torch.float32, return_parts=False):
        """scores [B]; with return_parts=True (score, lm, dm, query vector [B, H], pooled map [B, H, L - 101]).  No axis is squeezed by
        position: any batch size runs."""
        self._check(documents, queries)
        lm, dm, p = self.lm, self.dm, self.p
        act = torch.tanh if p["activation"] == "tanh" else F.relu
        B, L = documents.shape
        H = p["nfilters"]

        def wb(layer):
            return layer.weight.to(dtype), layer.bias.to(dtype)

        # local model
        match = (queries[:, :, None] == documents[:, None, :]).to(dtype)                       # [B, Q, L]
        if p["idfweight"]:
            match = match * query_idf[:, :, None].to(dtype)
        w, b = wb(lm.conv[0])
        x = act(torch.matmul(match, w.view(H, L).t()) + b).transpose(1, 2)                     # [B, H, Q]
        x = lm.ffw[2](act(F.linear(x.reshape(B, -1), *wb(lm.ffw[0]))))
        lm_score = F.linear(x, *wb(lm.ffw[3])).view(B)
        # distributed model: a (3, dim) convolution over rows is a linear map of three consecutive rows, flattened
        def conv3(rows, layer):                                                                 # [B, T, dim] -> [B, H, T - 2]
            w, b = wb(layer)
            win = torch.cat([rows[:, :-2], rows[:, 1:-1], rows[:, 2:]], dim=2)                  # [B, T - 2, 3 dim]
            return act(F.linear(win, w.view(H, -1), b)).transpose(1, 2)

        q = dm.q_conv[2](conv3(dm.embedding(queries).to(dtype), dm.q_conv[0]))
        qv = F.linear(F.max_pool1d(q, 2, 1).view(B, H), *wb(dm.q_ffw[0]))                      # [B, H]  (Q = 4: one pooled window)
        c = dm.d_conv1[2](conv3(dm.embedding(documents).to(dtype), dm.d_conv1[0]))
        pooled = F.max_pool1d(c, POOL, 1)                                                       # [B, H, L - 101]
        w, b = wb(dm.d_conv2[0])
        e = dm.d_conv2[2](act(torch.matmul(w.view(H, H), pooled) + b[None, :, None]))          # [B, H, L - 101]
        f = act(F.linear(qv[:, :, None] * e, *wb(dm.ffw_1[0]))).view(B, H)
        dm_score = F.linear(dm.ffw_2[0](f), *wb(dm.ffw_2[1])).view(B)
        score = lm_score + dm_score
        return (score, lm_score, dm_score, qv, pooled) if return_parts else score


class DUET(Reranker):
    """Bhaskar Mitra, Fernando Diaz, and Nick Craswell. 2017. Learning to Match using Local and Distributed Representations of Text for
    Web Search. In WWW'17.  (reference capreolus/reranker/DUET.py)"""

    module_name = "DUET"
    supports_resident = True   # term-id rows: served from a device-resident CandidateStore (Reranker.test_resident)
    supports_lists = False
    config_spec = {"nfilters": 10, "lmhidden": 30, "nhidden": 699, "idfweight": True, "dropoutrate": 0.5, "activation": "relu"}

    def build_model(self):
        if not hasattr(self, "model"):
            c = self.config
            D = np.asarray(self.extractor.embeddings).shape[1]
            ec = self.extractor.config
            check_geometry(ec["maxqlen"], ec["maxdoclen"], c["nfilters"], c["nhidden"])
            if int(c["nfilters"]) > MAX_FILTERS or not 1 <= int(c["lmhidden"]) <= MAX_LMHIDDEN or not 1 <= D <= MAX_DIM or int(ec["maxdoclen"]) > MAX_DOCLEN:
                raise ValueError(f"DUET takes nfilters <= {MAX_FILTERS}, lmhidden 1..{MAX_LMHIDDEN}, embeddings of dim <= {MAX_DIM} and maxdoclen <= "
                                 f"{MAX_DOCLEN}; got nfilters {c['nfilters']}, lmhidden {c['lmhidden']}, dim {D}, maxdoclen {ec['maxdoclen']}")
            _activation(c["activation"])
            self.model = DUET_class(self.extractor, self.config)
        return self.model

    def score(self, d):
        query_idf = d["query_idf"]
        query_sentence = d["query"]
        pos_sentence, neg_sentence = d["posdoc"], d["negdoc"]
        return [self.model(pos_sentence, query_sentence, query_idf).view(-1), self.model(neg_sentence, query_sentence, query_idf).view(-1)]

    def test(self, d):
        return self.model(d["posdoc"], d["query"], d["query_idf"]).view(-1)

    def zero_grad(self, *args, **kwargs):
        self.model.zero_grad(*args, **kwargs)
