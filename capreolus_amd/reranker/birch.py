"""Birch behind the reference plugin surface (capreolus/reranker/birch.py:35-161): the gfx950 BERT encoder of ptBERTMaxP scores the
passages (BertForNextSentencePrediction is that encoder's pooler and a [2, hidden] classifier under another name), csrc/birch.hip
decides which passages are encoded and how (capamd_birch_plan) and turns their logits into the document score (capamd_birch_head:
fill, top-k, combine), through the C ABI.

The module holds the parameters under the reference's state_dict names (``bert.bert.*``, ``bert.cls.seq_relationship.*``,
``combine.weight`` or ``combine.0.*`` / ``combine.2.*``), so reference checkpoints load unchanged.

What the reference computes, restated as written: only passages with more than two tokens of an attended segment B are encoded; they
run in sub-batches of `batch size` passages, each cut behind ``(seg + mask).argmax(dim=1).max()`` (:106-109).  argmax returns the FIRST
maximal position - the first token of segment B - so every passage is scored on ``[CLS] q [SEP] t1`` alone, and the cut of a passage
depends on the other passages of its sub-batch and on the batch size.  ``truncate = "reference"`` (default) reproduces exactly that;
``truncate = "none"`` scores the whole passage, as the paper and the commented-out loop (:110-115) have it, and a document's score then
depends on nothing but the document.
"""
import torch
from torch import nn

from .. import engine
from . import Reranker
from .ptBERTMaxP import _Box, bert_body

PRETRAINED = ("mb", "msmarco_mb", "car_mb")      # birch.py:138: Capreolus/birch-bert-large-{pretrained}


class Birch_Class(nn.Module):
    def __init__(self, extractor, config):
        super().__init__()
        self.extractor = extractor
        self.config = dict(config)
        topk, hidden = int(config["topk"]), int(config["hidden"])
        P, S = extractor.config["numpassages"], extractor.config["maxseqlen"]
        if topk > P:
            raise ValueError(f"topk = {topk} is larger than the extractor's numpassages = {P} (torch.topk over a document's passage scores, birch.py:81)")
        if config.get("truncate", "reference") not in engine.BIRCH_TRUNCATE:
            raise ValueError(f"truncate must be one of {sorted(engine.BIRCH_TRUNCATE)}; got {config['truncate']!r}")
        engine.BirchEngine.check_dims(P, S, topk, hidden)
        if hidden == 0:
            self.combine = nn.Linear(topk, 1, bias=False)
            with torch.no_grad():
                self.combine.weight.copy_(torch.ones_like(self.combine.weight) / topk)      # (the reference's expression, :44)
        else:
            self.combine = nn.Sequential(nn.Linear(topk, hidden), nn.ReLU(), nn.Linear(hidden, 1))
        pre = config["pretrained"]
        if isinstance(pre, dict):            # explicit geometry, weights loaded later with load_state_dict
            self.bert = self._container(**pre)
        else:
            self.bert = self._from_hf(pre)
        self.num_passages, self.maxseqlen = P, S
        self._engine = None

    @staticmethod
    def _container(hidden=1024, layers=24, heads=16, ffn=4096, vocab=30522, max_pos=512, type_vocab=2):
        """Parameter tree of transformers.BertForNextSentencePrediction (state_dict names as HF); BERT-large by default."""
        body = bert_body(hidden, layers, heads, ffn, vocab, max_pos, type_vocab)
        box = _Box(bert=body, cls=_Box(seq_relationship=nn.Linear(hidden, 2)))
        box.num_attention_heads = heads
        return box

    @classmethod
    def _from_hf(cls, name):
        """Reads a local/cached HF checkpoint (no network here) and copies its tensors into the container."""
        from transformers import BertForNextSentencePrediction

        if name in PRETRAINED:
            name = f"Capreolus/birch-bert-large-{name}"
        hf = BertForNextSentencePrediction.from_pretrained(name)
        c = hf.config
        if c.model_type != "bert" or c.hidden_act != "gelu":
            raise NotImplementedError(f"{name}: unsupported architecture {c.model_type}/{c.hidden_act}")
        box = cls._container(c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size, c.vocab_size,
                             c.max_position_embeddings, c.type_vocab_size)
        missing = box.load_state_dict(hf.state_dict(), strict=False)
        if missing.missing_keys:
            raise RuntimeError(f"checkpoint lacks {missing.missing_keys}")
        return box

    def _bert_params(self):
        """the encoder engine's names: the next-sentence head is its classifier"""
        p = {k: v for k, v in self.bert.state_dict(keep_vars=True).items() if not k.endswith("position_ids")}
        q = {k: v for k, v in p.items() if k.startswith("bert.")}
        q["classifier.weight"], q["classifier.bias"] = p["cls.seq_relationship.weight"], p["cls.seq_relationship.bias"]
        return q

    def combine_params(self):
        """combine's live tensors under their state_dict names (engine.BirchEngine.head reads them in place)"""
        return {"combine." + k: v for k, v in self.combine.state_dict(keep_vars=True).items()}

    def engine(self):
        if self._engine is None:
            be = engine.BertEngine(self._bert_params(), self.bert.num_attention_heads, microbatch=int(self.config.get("microbatch", 256)),
                                   compute_dtype=self.config.get("compute_dtype", "fp16"), skip_padding=bool(self.config.get("skip_padding", True)))
            self._engine = engine.BirchEngine(be, truncate=self.config.get("truncate", "reference"))
        else:
            self._engine.be.params = self._bert_params()
        return self._engine

    def forward(self, doc, seg, mask, subbatch=None):
        """(the reference's argument order, birch.py:72: seg BEFORE mask)  subbatch: the passages per sub-batch under truncate =
        "reference"; default the call's batch size, as in the reference."""
        if self.training and self.config.get("finetune", False):
            raise NotImplementedError(
                "capreolus_amd scores with hand-written inference kernels; fine-tuning the encoder (birch.py:66-70, finetune = True) is "
                "not part of this engine.  finetune = False trains `combine` on the engine's top-k passage scores."
            )
        B = doc.shape[0]
        shape = (B, self.num_passages, self.maxseqlen)
        doc, seg, mask = doc.reshape(shape), seg.reshape(shape), mask.reshape(shape)
        topk = int(self.config["topk"])
        if not self.training:
            return self.engine().forward(doc, mask, seg, topk, self.combine_params(), subbatch=subbatch).view(-1, 1)
        # finetune = False: the encoder runs without a graph (birch.py:66-68, 75), `combine` is all that trains - the plain nn module
        # on the engine's top-k values
        with torch.no_grad():
            top = self.engine().forward(doc, mask, seg, topk, self.combine_params(), subbatch=subbatch, details=True)[1]
        return self.combine(top.detach())


class Birch(Reranker):
    """Yilmaz, Yang, Zhang, Lin. Cross-Domain Modeling of Sentence-Level Evidence for Document Retrieval. EMNLP 2019 (reference
    birch.py:130-161).  The first four keys are the reference's options; microbatch / compute_dtype / skip_padding belong to the encoder
    engine (as in ptBERTMaxP); truncate: "reference" (the cut of birch.py:106-109 as written) or "none" (the whole passage)."""

    module_name = "birch"
    config_spec = {"topk": 3, "hidden": 0, "finetune": False, "pretrained": "msmarco_mb", "microbatch": 256, "compute_dtype": "fp16",
                   "skip_padding": True, "truncate": "reference"}

    @property
    def batch_coupled(self):
        """truncate = "reference": the sub-batches hold `batch size` passages (birch.py:73-76, 98-103), so a passage's cut - and its
        score - depends on the batch it arrives in; `PytorchTrainer.predict` must not merge DataLoader batches then."""
        return self.config["truncate"] == "reference"

    def build_model(self):
        if not hasattr(self, "model"):
            self.model = Birch_Class(self.extractor, self.config)
        return self.model

    def score(self, d):
        return [self.model(d["pos_bert_input"], d["pos_seg"], d["pos_mask"]).view(-1),
                self.model(d["neg_bert_input"], d["neg_seg"], d["neg_mask"]).view(-1)]

    def test(self, d):
        return self.model(d["pos_bert_input"], d["pos_seg"], d["pos_mask"]).view(-1)
