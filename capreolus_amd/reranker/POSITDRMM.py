"""POSITDRMM (McDonald et al., EMNLP'18), behind the reference plugin surface (capreolus/reranker/POSITDRMM.py).

The module tree carries the reference's state_dict names (``posit1.embedding.weight``, ``posit1.encoding_layer.{weight_ih,weight_hh,
bias_ih,bias_hh}_l{0,1}{,_reverse}``, ``posit1.Q1.{weight,bias}``, ``posit1.Wg.{weight,bias}``), so checkpoints interchange in both
directions; ``encoding_layer`` is a real nn.LSTM(D, D, num_layers=2, bidirectional=True, dropout=0.3).  Scoring (`test`, eval-mode
forward) is one C-ABI call (capamd_posit_forward, csrc/posit.hip) in fp32; training mode with grad enabled runs the restatement below
under autograd, with the module's own nn.LSTM and both dropouts as the reference does.

Semantics (reference POSITDRMM.py), quirks included:
  - M_cos = (q / (|q| + 1e-7)) . (d / (|d| + 1e-7)): each side normalised on its own; the context cosine has NO epsilon;
  - the exact-match matrix is 1 where the ids are equal and is zeroed only where the QUERY id equals extractor.pad (a document pad never
    equals a non-pad query id);
  - the LSTM starts from zero state for the query and for the document (the reference assigns self.hidden but never passes it in) and
    runs over all positions, pads included: the outputs at pad positions are non-zero and take part in the max and the top-5;
  - the residual is added per direction: context = [fwd + x, bwd + x];
  - six features per query term: the max and the mean of the 5 largest over the document axis of M_cos, M_cos_context and the
    exact-match matrix; Q1, LeakyReLU(0.01), a sum weighted by softmax(query_idf), Wg over [ans, extras(4)];
  - the extras are [exact matches / len, idf-weighted exact matches / len, bigram matches / (len - 1), the searcher's score], where the
    query is taken as it is (pads included) and the document without its pads (len = its non-pad terms; a bigram may span a removed
    pad); the counts are integers, the idf sum runs over the query positions in order in fp32.

Differences from the reference, only where it cannot run:
  - any batch size is taken (the reference needs exactly trainer.config["batch"] pairs); Q and L come from the tensors;
  - L < 5 is refused with ValueError (its topk fails), a document of fewer than 2 non-pad terms is refused with ValueError by the match
    statistics (it divides by zero or stacks an empty bigram list; a query of one term, whose bigram list is empty too, counts 0 bigram
    matches here), and an embedding dim above the kernel's limit is refused with ValueError.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import engine
from . import Reranker

# the limits of capamd_posit_forward (include/capreolus_amd.h)
MAX_DIM, MAX_QLEN, MIN_DOCLEN, MAX_DOCLEN = 320, 16, 5, 8192


def exact_match_stats(query_idf, query, doc, pad):
    """The reference's get_exact_match_stats (its loops per pair, per query word and per bigram) as tensor operations on the device of
    the ids: three [B, 1] fp32 columns.  Integer counts; the divisions as the reference rounds them (Python floats stored to fp32 for the
    two counts, an fp32 division for the idf sum)."""
    query, doc = query.long(), doc.long()
    Q, L = query.shape[1], doc.shape[1]
    nonpad = doc != pad
    length = nonpad.sum(1)
    if bool((length < 2).any()):
        raise ValueError("POSITDRMM: a document has fewer than 2 non-pad terms (the reference's match statistics divide by its length and "
                         "by its number of bigrams)")
    counts = ((query[:, :, None] == doc[:, None, :]) & nonpad[:, None, :]).sum(2)          # [B, Q]
    widf = torch.zeros(doc.shape[0], dtype=torch.float32, device=doc.device)
    for i in range(Q):
        widf = widf + counts[:, i].to(torch.float32) * query_idf[:, i].to(torch.float32)
    # the cleaned document, packed to the left
    cleaned = doc.gather(1, torch.argsort((~nonpad).to(torch.int8), dim=1, stable=True))
    live = torch.arange(L - 1, device=doc.device)[None, :] < (length - 1)[:, None]
    bigrams = ((query[:, :-1, None] == cleaned[:, None, :-1]) & (query[:, 1:, None] == cleaned[:, None, 1:]) & live[:, None, :]).sum((1, 2))
    s0 = (counts.sum(1).double() / length.double()).to(torch.float32)
    s1 = widf / length.to(torch.float32)
    s2 = (bigrams.double() / (length - 1).double()).to(torch.float32)
    return s0.reshape(-1, 1), s1.reshape(-1, 1), s2.reshape(-1, 1)


class POSITDRMM_basic(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        weights = torch.as_tensor(np.asarray(extractor.embeddings, dtype=np.float32))
        self.embedding_dim = self.lstm_hidden_dim = weights.shape[1]
        self.encoding_layer = nn.LSTM(input_size=self.embedding_dim, hidden_size=self.embedding_dim, num_layers=2, bidirectional=True, dropout=0.3)
        self.pad_token = extractor.pad
        self.embedding = nn.Embedding(*weights.shape)
        self.embedding.weight.data.copy_(weights)
        self.embedding.weight.requires_grad = False
        self.m = nn.Dropout(p=0.2)
        self.Q1 = nn.Linear(6, 1, bias=True)
        self.Wg = nn.Linear(5, 1)
        self.activation = nn.LeakyReLU()

    def forward(self, sentence, query_sentence, query_idf, extra, dtype=torch.float32, return_details=False):
        """the reference's POSITDRMM_basic.forward in `dtype`: [B] scores (and a dict of the [B, Q, 6] input of Q1 and the two context
        tensors).  fp32 runs the module's own nn.LSTM (under autograd in training, with both dropouts); any other dtype runs a copy of it
        in that dtype."""
        if sentence.shape[1] < MIN_DOCLEN:
            raise ValueError(f"POSITDRMM takes documents of at least {MIN_DOCLEN} positions (the mean of the top 5); got L {sentence.shape[1]}")
        lstm = self.encoding_layer if dtype == torch.float32 else copy.deepcopy(self.encoding_layer).to(dtype)
        x, query_x = self.embedding(sentence).to(dtype), self.embedding(query_sentence).to(dtype)
        x_norm = x / (x.norm(dim=2)[:, :, None] + 1e-7)
        query_x_norm = query_x / (query_x.norm(dim=2)[:, :, None] + 1e-7)
        M_cos = torch.matmul(query_x_norm, x_norm.transpose(1, 2))
        xor = (query_sentence[:, :, None] == sentence[:, None, :]) & (query_sentence[:, :, None] != self.pad_token)
        xor = xor.to(dtype)
        H = self.lstm_hidden_dim

        def context(e):                                                    # [B, S, D] -> [B, S, 2 D], from zero state
            e = e.transpose(0, 1)
            p1, _ = lstm(self.m(e))
            return torch.cat([p1[:, :, :H] + e, p1[:, :, H:] + e], dim=2).transpose(0, 1)

        query_context, doc_context = context(query_x), context(x)
        M_ctx = torch.matmul(query_context / query_context.norm(dim=2)[:, :, None], (doc_context / doc_context.norm(dim=2)[:, :, None]).transpose(1, 2))
        feats = []
        for M in (M_cos, M_ctx, xor):
            feats += [M.max(2)[0], torch.topk(M, 5, dim=2)[0].sum(2) / 5]
        M_max = torch.stack(feats, dim=2)                                  # [B, Q, 6]
        M_res = self.activation(F.linear(M_max, self.Q1.weight.to(dtype), self.Q1.bias.to(dtype)))[:, :, 0]
        ans = (F.softmax(query_idf.to(dtype), dim=1) * M_res).sum(1).view(-1, 1)
        score = F.linear(torch.cat([ans, extra.to(dtype)], dim=1), self.Wg.weight.to(dtype), self.Wg.bias.to(dtype)).view(-1)
        if return_details:
            return score, {"features": M_max, "query_context": query_context, "doc_context": doc_context}
        return score


class POSITDRMM_class(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.posit1 = POSITDRMM_basic(extractor, config)
        self.p = config
        self._engine = engine.PositEngine()

    def _params(self):
        return dict(self.named_parameters())

    def test_forward(self, query_sentence, query_idf, pos_sentence, extras):
        """[B] scores"""
        if torch.is_grad_enabled() and self.training:
            return self._forward_aten(pos_sentence, query_sentence, query_idf, extras)
        return self.forward_engine(pos_sentence, query_sentence, query_idf, extras=extras)

    def forward(self, query_sentence, query_idf, pos_sentence, neg_sentence, posdoc_extra, negdoc_extra):
        return [self.test_forward(query_sentence, query_idf, pos_sentence, posdoc_extra),
                self.test_forward(query_sentence, query_idf, neg_sentence, negdoc_extra)]

    def forward_engine(self, doctoks, querytoks, query_idf, extras=None, bm25=None, details=False):
        """capamd_posit_forward: fp32 scores [B] from extras [B, 4], or from bm25 [B] and the kernel's own match statistics (with
        details=True also the features, the statistics and the two context tensors)"""
        if doctoks.shape[1] < MIN_DOCLEN:
            raise ValueError(f"POSITDRMM takes documents of at least {MIN_DOCLEN} positions (the mean of the top 5); got L {doctoks.shape[1]}")
        return self._engine.forward(querytoks, query_idf, doctoks, self._params(), self.posit1.pad_token, extras=extras, bm25=bm25, details=details)

    def _forward_aten(self, doctoks, querytoks, query_idf, extras, dtype=torch.float32, return_details=False):
        """the restatement: under autograd in training; in float64 in eval mode it is what the tests hold the kernels against"""
        return self.posit1(doctoks, querytoks, query_idf, extras, dtype=dtype, return_details=return_details)


class POSITDRMM(Reranker):
    """Ryan McDonald, George Brokos, and Ion Androutsopoulos. 2018. Deep Relevance Ranking Using Enhanced Document-Query Interactions.
    In EMNLP'18.  (reference capreolus/reranker/POSITDRMM.py)"""

    module_name = "POSITDRMM"
    supports_resident = False    # `test` needs qid / posdocid for the searcher's scores
    supports_lists = False
    config_spec = {}

    def build_model(self):
        if not hasattr(self, "model"):
            D = np.asarray(self.extractor.embeddings).shape[1]
            if D > MAX_DIM:
                raise ValueError(f"POSITDRMM takes embeddings of dim <= {MAX_DIM}; got dim {D}")
            config = dict(self.config)
            config.update(getattr(self.extractor, "config", None) or {})
            self.model = POSITDRMM_class(self.extractor, config)
        return self.model

    def get_searcher_scores(self, qids, doc_ids):
        # the searcher_scores attribute is set by the rerank task before training, as in the reference
        return torch.tensor([float(self.searcher_scores[q][doc_id]) for q, doc_id in zip(qids, doc_ids)], dtype=torch.float32).reshape(-1, 1)

    def get_exact_match_stats(self, query_idf_batch, query_batch, doc_batch):
        return exact_match_stats(query_idf_batch, query_batch, doc_batch, self.extractor.pad)

    def _extras(self, d, doc_key, docid_key):
        stats = self.get_exact_match_stats(d["query_idf"], d["query"], d[doc_key])
        return torch.cat(stats + (self.get_searcher_scores(d["qid"], d[docid_key]).to(d[doc_key].device),), dim=1)

    def score(self, d):
        return self.model(d["query"], d["query_idf"], d["posdoc"], d["negdoc"], self._extras(d, "posdoc", "posdocid"),
                          self._extras(d, "negdoc", "negdocid"))

    def test(self, d):
        if d["posdoc"].is_cuda and not (torch.is_grad_enabled() and self.model.training):
            # one call: the match statistics are formed by the kernel that reads the ids anyway
            bm25 = self.get_searcher_scores(d["qid"], d["posdocid"]).to(d["posdoc"].device)
            return self.model.forward_engine(d["posdoc"], d["query"], d["query_idf"], bm25=bm25.view(-1))
        return self.model.test_forward(d["query"], d["query_idf"], d["posdoc"], self._extras(d, "posdoc", "posdocid"))

    def zero_grad(self, *args, **kwargs):
        self.model.zero_grad(*args, **kwargs)
