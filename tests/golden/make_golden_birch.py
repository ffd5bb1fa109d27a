"""Birch golden vectors: the REFERENCE Birch_Class (capreolus/reranker/birch.py, imported from the reference tree through _refharness)
driving transformers' BertForNextSentencePrediction on seeded weights (tests/birch_case.py) and seeded BirchBertPassage-shaped inputs.
Build container only; data out, no code.

    python tests/golden/make_golden_birch.py            (from the repository root)

Stored per fixture: the inputs (int32 / int8), the reference's scores, the passage logits its sub-batches produced (a hook on
model.bert; the order of the sub-batches is the order of the compacted rows), both again under torch.autocast("cpu") in fp16 and bf16,
the same model's logits on the FULL valid passages (what truncate = "none" scores), the shapes the sub-batches had, and the state_dict
keys.  Only the weights' seed is stored.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import birch_case  # noqa: E402

CLS, SEP, PAD = 101, 102, 0
MINI = dict(hidden=128, layers=2, heads=2, ffn=512, vocab=1000, max_pos=128)
CASES = {
    "birch_mini": dict(MINI, B=5, P=6, S=64, topk=3, combine_hidden=0, seed=31, inputs="counts", head_scale=4.0),
    "birch_hidden": dict(MINI, B=5, P=6, S=64, topk=2, combine_hidden=8, seed=31, inputs="counts", head_scale=4.0),
    "birch_mixed": dict(MINI, B=4, P=5, S=64, topk=3, combine_hidden=0, seed=33, inputs="mixed", head_scale=4.0),
    # BERT-large's width (1024 hidden, 16 heads, 4096 FFN) at two layers
    "birch_wide": dict(hidden=1024, layers=2, heads=16, ffn=4096, vocab=1000, max_pos=128, B=3, P=4, S=64, topk=2, combine_hidden=0, seed=34,
                       inputs="wide", head_scale=1.0),
}


def passage(q, body, S, holes=()):
    """`[CLS] q [SEP] body [SEP] [PAD]...` as (ids, mask, seg) rows: mask = 1 on non-pad tokens (0 at `holes`), seg = 1 from the first body
    token to the END of the row, pads included (bertpassage.py:268-284; an empty passage's body is one [PAD])"""
    toks = [CLS] + list(q) + [SEP] + list(body) + [SEP]
    assert len(toks) <= S
    ids, mask, seg = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)
    ids[:len(toks)] = toks
    mask[:len(toks)] = [0 if t == PAD else 1 for t in toks]
    mask[list(holes)] = 0
    seg[len(q) + 2:] = 1
    return ids, mask, seg


def make_inputs(kind, rs, B, P, S, vocab):
    """[B, P, S] x3.  counts: documents with P, 0, 1, 2 and 4 valid passages (the 6 of the first make two sub-batches of 5 and 1).
    mixed: passages of one document under queries of different lengths (a sub-batch's cut is then not every row's own), bodies of exactly
    one, two (two 2s: not valid) and three tokens (three 2s: valid), a hole in a query and one in a body.  wide: plain."""
    tok = lambda n: list(rs.randint(vocab // 4, vocab, size=n))
    out = np.zeros((3, B, P, S), np.int64)
    for b in range(B):
        q = tok(rs.randint(3, 9))
        for p in range(P):
            body, holes, qq = tok(rs.randint(4, S - len(q) - 3)), (), q
            if kind == "counts":
                keep = {0: range(P), 1: (), 2: (2,), 3: (1, 4), 4: (0, 2, 3, 5)}[b]
                if p not in keep:
                    body = [PAD]
            elif kind == "mixed":
                if b == 0:
                    qq = q[:2 + p]                                     # query lengths 2 .. 6 inside one document
                    body = tok(rs.randint(4, S - len(qq) - 3))
                elif b == 1:
                    body = [tok(1), tok(2), tok(3), [PAD], tok(20)][p]   # 1, 2, 3 twos (the [SEP] counts), an empty passage, a plain one
                elif b == 2 and p == 1:
                    holes = (2,)                                       # a hole in the query
                elif b == 2 and p == 3:
                    holes = (len(q) + 5,)                              # a hole in the body
                elif b == 3 and p in (1, 2):
                    qq = q + tok(4) if p == 1 else q[:3]
                    body = tok(rs.randint(4, S - len(qq) - 3))
            out[:, b, p] = passage(qq, body, S, holes)
    return out


def run_reference(model, ids, seg, mask, amp=None):
    """-> (scores [B], the sub-batches' logit 1 concatenated, their shapes)"""
    seen, shapes = [], []

    def spy(module, args, kwargs, output):
        seen.append(output[0][:, 1].detach().float())
        shapes.append(tuple(kwargs["input_ids"].shape))

    hook = model.bert.register_forward_hook(spy, with_kwargs=True)
    try:
        with torch.no_grad():
            if amp is None:
                score = model(ids, seg, mask)
            else:
                with torch.autocast("cpu", dtype=amp):       # the reference's amp = pred mode, on the CPU
                    score = model(ids, seg, mask)
    finally:
        hook.remove()
    return score.view(-1).float().numpy(), torch.cat(seen).numpy(), np.array(shapes, dtype=np.int64)


def build_model(c, BIRCH):
    from transformers import BertConfig, BertForNextSentencePrediction

    cfg = BertConfig(hidden_size=c["hidden"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"], intermediate_size=c["ffn"],
                     vocab_size=c["vocab"], max_position_embeddings=c["max_pos"])
    orig = BertForNextSentencePrediction.from_pretrained
    BertForNextSentencePrediction.from_pretrained = staticmethod(lambda *a, **k: BertForNextSentencePrediction(cfg))
    try:
        model = BIRCH.Birch_Class(None, {"topk": c["topk"], "hidden": c["combine_hidden"], "finetune": False, "pretrained": "seeded",
                                         "extractor": {"numpassages": c["P"]}})
    finally:
        BertForNextSentencePrediction.from_pretrained = orig
    if c["combine_hidden"] == 0:       # the reference's own initialisation is part of the fixture
        assert torch.equal(model.combine.weight, torch.ones(1, c["topk"]) / c["topk"])
    dims = [c[k] for k in ("hidden", "layers", "heads", "ffn", "vocab", "max_pos")]
    missing = model.bert.load_state_dict(birch_case.birch_weights(c["seed"], dims, c["head_scale"]), strict=False)
    assert not missing.unexpected_keys and not [k for k in missing.missing_keys if "position_ids" not in k], missing
    combine = birch_case.birch_combine_weights(c["seed"], c["topk"], c["combine_hidden"])
    model.load_state_dict(combine, strict=False)
    return model.eval(), dims, combine


def full_logits(model, ids, seg, mask, rows, amp=None):
    b, p = (torch.tensor(x) for x in zip(*rows))
    with torch.no_grad():
        if amp is None:
            return model.bert(input_ids=ids[b, p], token_type_ids=seg[b, p], attention_mask=mask[b, p])[0][:, 1].float().numpy()
        with torch.autocast("cpu", dtype=amp):
            return model.bert(input_ids=ids[b, p], token_type_ids=seg[b, p], attention_mask=mask[b, p])[0][:, 1].float().numpy()


def spread_ok(scores, bound):
    """at least half of the document pairs differ by more than twice the end-to-end bound: the rank check judges only such pairs"""
    n = len(scores)
    far = sum(abs(scores[i] - scores[j]) > 2 * bound for i in range(n) for j in range(i + 1, n))
    return far * 2 >= n * (n - 1) // 2, far


def gen(name, c, BIRCH):
    B, P, S = c["B"], c["P"], c["S"]
    model, dims, combine = build_model(c, BIRCH)
    ids, mask, seg = (torch.from_numpy(x) for x in make_inputs(c["inputs"], np.random.RandomState(c["seed"]), B, P, S, c["vocab"]))
    ref, logits, shapes = run_reference(model, ids, seg, mask)
    plan = birch_case.plan_restated(mask.numpy(), seg.numpy(), B, "reference")
    assert [tuple(s) for s in shapes] == [(n, cut + 1) for n, cut in _subbatches(plan, B)], (shapes, list(_subbatches(plan, B)))
    # (1) the float64 restatement fed the reference's own logits reproduces its score to fp32 rounding
    got, _, _ = birch_case.head_restated(logits, plan["doc_first"], P, c["topk"], combine)
    assert np.abs(got - ref).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(ref).max()) * max(1, c["combine_hidden"]), (name, got, ref)
    out = dict(ref_score=ref, ref_enc_logits=logits, subbatch_shapes=shapes)
    for dt, tag in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        s, l, sh = run_reference(model, ids, seg, mask, amp=dt)
        assert np.array_equal(sh, shapes)
        out[f"ref_score_amp_{tag}"], out[f"ref_enc_logits_amp_{tag}"] = s, l
        out[f"ref_full_logits_amp_{tag}"] = full_logits(model, ids, seg, mask, plan["rows"], amp=dt)
    out["ref_full_logits"] = full_logits(model, ids, seg, mask, plan["rows"])
    # (2) the documents' scores spread over the end-to-end bound (fp16, the default operand type), in both modes
    for mode, key in (("reference", "ref_enc_logits"), ("none", "ref_full_logits")):
        eps = birch_case.E2E_FACTOR["fp16"] * np.abs(out[key + "_amp_fp16"] - out[key]).max() + 1e-4
        sc = birch_case.head_restated(out[key], plan["doc_first"], P, c["topk"], combine)[0]
        ok, far = spread_ok(sc, birch_case.score_bound(combine, eps))
        assert ok, (name, mode, far, sc, eps)
        print(name, mode, "scores", np.round(sc, 4), "logit bound", eps, "pairs judged", far)
    sd = model.state_dict()
    keys = sorted(k for k in sd if not k.endswith("position_ids"))
    np.savez_compressed(
        os.path.join(HERE, f"{name}.npz"), weight_seed=np.int64(c["seed"]), dims=np.array(dims, dtype=np.int64), P=np.int64(P), S=np.int64(S),
        topk=np.int64(c["topk"]), hidden=np.int64(c["combine_hidden"]), head_scale=np.float64(c["head_scale"]),
        pos_bert_input=ids.numpy().astype(np.int32), pos_mask=mask.numpy().astype(np.int8), pos_seg=seg.numpy().astype(np.int8),
        state_keys=np.array(keys), **{k: (v.astype(np.float32) if v.dtype.kind == "f" else v) for k, v in out.items()})
    return model, (ids, mask, seg), out, plan, combine


def _subbatches(plan, subbatch):
    """(rows, cut) of every sub-batch, in order"""
    df = plan["doc_first"]
    for b in range(len(df) - 1):
        for r0 in range(df[b], df[b + 1], subbatch):
            yield min(subbatch, df[b + 1] - r0), int(plan["cut"][r0])


def gen_grad(made, BIRCH):
    """`combine`'s gradients of the reference's pairwise step (trainer/pytorch.py:93-102 with softmaxloss: reranker/common.py:96-98) with
    finetune = False: the fixture's documents as the positive ones, a second seeded batch as the negative ones."""
    common = importlib.import_module("capreolus.reranker.common")
    out = {}
    for name in birch_case.GRAD_CASES:
        c = CASES[name]
        model, (ids, mask, seg), fx, plan, combine = made[name]
        B, P, S = c["B"], c["P"], c["S"]
        nids, nmask, nseg = (torch.from_numpy(x) for x in make_inputs(c["inputs"], np.random.RandomState(c["seed"] + 500), B, P, S, c["vocab"]))
        _, nlog, _ = run_reference(model, nids, nseg, nmask)
        _, nlog16, _ = run_reference(model, nids, nseg, nmask, amp=torch.float16)
        nplan = birch_case.plan_restated(nmask.numpy(), nseg.numpy(), B, "reference")
        model.zero_grad()
        loss = common.pair_softmax_loss([model(ids, seg, mask).view(-1), model(nids, nseg, nmask).view(-1)])
        loss.backward()
        assert all(p.grad is None for p in model.bert.parameters())
        grads = {"combine." + k: p.grad.numpy().astype(np.float64) for k, p in model.combine.named_parameters()}
        tp = birch_case.head_restated(fx["ref_enc_logits"], plan["doc_first"], P, c["topk"], combine)[1]
        tn = birch_case.head_restated(nlog, nplan["doc_first"], P, c["topk"], combine)[1]
        want, _, _ = birch_case.grad_restated(tp, tn, combine)
        for k in grads:
            assert np.abs(grads[k] - want[k]).max() <= 1e-6, (name, k, grads[k], want[k])
        eps = birch_case.E2E_FACTOR["fp16"] * max(np.abs(fx["ref_enc_logits_amp_fp16"] - fx["ref_enc_logits"]).max(), np.abs(nlog16 - nlog).max()) + 1e-4
        assert birch_case.relu_margin_ok(tp, tn, combine, eps), (name, "a hidden unit sits within the bound of its kink: change the inputs' seed")
        bound = birch_case.grad_bound(tp, tn, combine, eps)
        print(name, "loss", float(loss), "eps", eps, {k: (float(np.abs(v).max()), float(bound[k].max())) for k, v in grads.items()})
        out.update({f"{name}.neg_bert_input": nids.numpy().astype(np.int32), f"{name}.neg_mask": nmask.numpy().astype(np.int8),
                    f"{name}.neg_seg": nseg.numpy().astype(np.int8), f"{name}.neg_enc_logits": nlog.astype(np.float32),
                    f"{name}.neg_enc_logits_amp_fp16": nlog16.astype(np.float32), f"{name}.loss": np.float32(float(loss))})
        out.update({f"{name}.grad.{k}": v.astype(np.float32) for k, v in grads.items()})
    np.savez_compressed(os.path.join(HERE, "birch_grad.npz"), **out)


def main(only=None):
    import _refharness

    _refharness.load_reference()
    BIRCH = importlib.import_module("capreolus.reranker.birch")
    made = {name: gen(name, c, BIRCH) for name, c in CASES.items() if not only or name in only}
    if not only:
        gen_grad(made, BIRCH)


if __name__ == "__main__":
    main(sys.argv[1:])
