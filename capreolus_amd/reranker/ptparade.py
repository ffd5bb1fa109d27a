"""PARADE behind the reference plugin surface (capreolus/reranker/ptparade.py:81-117), aggregation = "transformer": the gfx950 BERT
encoder of ptBERTMaxP leaves the fp32 [CLS] row of every passage's last hidden state (csrc/bert.hip, capamd_parade_passage_cls), and
the aggregation head - two post-LN BertLayers over [initial_cls; passage rows] + position embeddings, then `linear` on row 0 - runs
in fp32 in csrc/parade.hip (capamd_parade_head), through the C ABI.

The module holds the parameters under the reference's state_dict names (``bert.embeddings.*``, ``bert.encoder.layer.N.*``,
``bert.pooler.dense.*`` for BERT bodies, ``transformer_layer_{1,2}.*`` with BertLayer's attribute tree, ``linear.*``,
``initial_cls_embedding``, ``full_position_embeddings``) so checkpoints interchange.  Encoders: BertModel checkpoints and ElectraModel
checkpoints whose embedding size equals the hidden size (electra-base-msmarco: the same encoder without a pooler), or an explicit
geometry (a dict of bert_body's arguments; ``pooler=False`` for an ELECTRA body).
"""
import torch
from torch import nn

from .. import engine
from . import Reranker
from .ptBERTMaxP import _encoder_layer, bert_body, encoder_from_hf

PRETRAINED = ("bert-base-uncased", "bert-base-msmarco", "electra-base-msmarco")   # ptparade.py:16-25
CLS_TOKEN_ID = 101                                                                 # ptparade.py:41-43 (hard-coded there too)


class PTParade_Class(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.extractor = extractor
        self.config = dict(config)
        pre = config["pretrained"]
        if isinstance(pre, dict):            # explicit geometry, weights loaded later with load_state_dict
            self.bert = bert_body(**pre)
        elif pre in PRETRAINED:
            self.bert = encoder_from_hf(pre, 0.1)
        else:
            raise ValueError(f"unsupported model: {pre}; need to ensure correct tokenizers will be used before arbitrary hgf models are supported")
        emb = self.bert.embeddings.word_embeddings.weight
        H, F = emb.shape[1], self.bert.encoder.layer[0].intermediate.dense.weight.shape[0]
        self.hidden_size = H
        self.transformer_layer_1 = _encoder_layer(H, F)
        self.transformer_layer_2 = _encoder_layer(H, F)
        self.num_passages = extractor.config["numpassages"]
        self.maxseqlen = extractor.config["maxseqlen"]
        self.linear = nn.Linear(H, 1)
        agg = config["aggregation"]
        if agg in ("max", "avg", "attn"):
            raise NotImplementedError(f"aggregation {agg} is not implemented (the reference raises too, ptparade.py:32-37)")
        if agg != "transformer":
            raise ValueError(f"unknown aggregation type: {agg}")
        init = emb.detach()[CLS_TOKEN_ID].clone() if emb.shape[0] > CLS_TOKEN_ID else torch.zeros(H)
        self.initial_cls_embedding = nn.Parameter(init.view(1, H))
        self.full_position_embeddings = nn.Parameter(torch.empty(1, self.num_passages + 1, H).normal_(mean=0.0, std=0.02))
        self._engine = None

    def _bert_params(self):
        return {"bert." + k: v for k, v in self.bert.state_dict(keep_vars=True).items() if not k.endswith("position_ids")}

    def head_params(self):
        """The aggregation head's live tensors under their state_dict names (engine.ParadeEngine.head reads them in place)."""
        return {k: v for k, v in self.state_dict(keep_vars=True).items() if not k.startswith("bert.")}

    def engine(self):
        if self._engine is None:
            be = engine.BertEngine(self._bert_params(), self.bert.num_attention_heads, microbatch=int(self.config.get("microbatch", 256)),
                                   compute_dtype=self.config.get("compute_dtype", "fp16"), skip_padding=bool(self.config.get("skip_padding", True)))
            self._engine = engine.ParadeEngine(be, ln_eps=self.transformer_layer_1.output.LayerNorm.eps)
        else:
            self._engine.be.params = self._bert_params()
        return self._engine

    def forward(self, doc_input, doc_mask, doc_seg):
        if self.training:
            raise NotImplementedError(
                "capreolus_amd scores with hand-written inference kernels; fine-tuning (ptBERTMaxP.py:60-61) is not part of "
                "this engine. Call under model.eval() as PytorchTrainer.predict does."
            )
        B = doc_input.shape[0]
        shape = (B, self.num_passages, self.maxseqlen)
        if self.num_passages > engine.PARADE_MAX_PASSAGES:
            raise ValueError(f"PARADE scores at most {engine.PARADE_MAX_PASSAGES} passages per document; got {self.num_passages}")
        out = self.engine().forward(doc_input.reshape(shape), doc_mask.reshape(shape), doc_seg.reshape(shape), self.head_params())
        return out.view(-1, 1)


class PTParade(Reranker):
    """Li, Yates, MacAvaney, He, Sun. PARADE: Passage Representation Aggregation for Document Reranking. arXiv 2020 (reference
    ptparade.py:81-117).  The first two keys are the reference's options; microbatch / compute_dtype / skip_padding belong to this engine
    (as in ptBERTMaxP)."""

    module_name = "ptparade"
    config_spec = {"pretrained": "bert-base-uncased", "aggregation": "transformer", "microbatch": 256, "compute_dtype": "fp16",
                   "skip_padding": True}

    def build_model(self):
        if not hasattr(self, "model"):
            self.model = PTParade_Class(self.extractor, self.config)
        return self.model

    def score(self, d):
        return [self.model(d["pos_bert_input"], d["pos_mask"], d["pos_seg"]).view(-1),
                self.model(d["neg_bert_input"], d["neg_mask"], d["neg_seg"]).view(-1)]

    def test(self, d):
        return self.model(d["pos_bert_input"], d["pos_mask"], d["pos_seg"]).view(-1)
