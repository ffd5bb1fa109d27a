"""The float64 restatement of CEDR-KNRM's similarity tap and document head (tests/cedr_case.py) against the fp32 port of the reference
module and the reference's own recorded scores: what the GPU tests of the tap (tests/test_gpu_cedr_tap.py) then rely on."""
import numpy as np
import pytest
import torch

from oracle import bert_port
from tests import cedr_case
from tests.helpers import load_cedr_case, rel_err


@pytest.mark.parametrize("name", ["mini", "mini_nocls"])
def test_restatement_matches_the_port_and_the_reference_scores(name):
    c, w, head, mus, sigmas = load_cedr_case(name)
    hidden, layers, heads = (int(c["dims"][i]) for i in (0, 1, 2))
    d = [torch.from_numpy(c[k].astype(np.int64)) for k in ("pos_bert_input", "pos_mask", "pos_seg")]
    B, P, S = d[0].shape
    A, sel = int(c["maxqlen"]) + 1, [int(x) for x in c["simmat_layers"]]
    ids, mask, seg = (t.reshape(B * P, S) for t in d)
    with torch.no_grad():
        hs = bert_port.encode_hidden(w, ids, mask, seg, heads, layers)
    qm0 = ((d[1][:, 0, 1:A + 1] != 0) & (d[2][:, 0, 1:A + 1] == 0)).float().repeat_interleave(P, dim=0)
    mu, sigma = torch.tensor(mus, dtype=torch.float32), torch.tensor(sigmas, dtype=torch.float32)
    pk = torch.stack([cedr_case.ref_pk(hs[li], mask, seg, qm0, A, mu, sigma) for li in sel])
    mode = {None: 0, "avg": 1, "max": 2}[c["cls_mode"]]
    w1, b1 = head["combine.0.weight"], head["combine.0.bias"]
    two = "combine.1.weight" in head
    scores, feats = cedr_case.ref_score(pk, hs[-1][:, 0], P, mode, w1 if two else w1.view(-1), b1,
                                        head["combine.1.weight"].view(-1) if two else None, head["combine.1.bias"] if two else None)
    n_in = w1.shape[1]
    eye = {"combine.0.weight": torch.eye(n_in), "combine.0.bias": torch.zeros(n_in)}       # the port with an identity head returns the features
    want = bert_port.cedr_knrm(w, eye, *d, heads, layers, A - 1, sel, mus, sigmas, c["cls_mode"]).view(B, n_in).double()
    err = (feats - want).abs().max().item()
    print(name, "features: max abs err", err, "of", want.abs().max().item())
    assert feats.shape == want.shape and err <= 1e-5 * want.abs().max().item()
    e = rel_err(scores.numpy(), c["ref_scores"])
    print(name, "scores: max rel err", e.max())
    assert e.max() <= 1e-4, (e, scores, c["ref_scores"])


def test_the_first_passages_query_mask_pools_and_the_passages_own_masks_the_similarities():
    """Two mask roles: a passage's OWN query mask zeroes its similarity rows (masked_simmats), the FIRST passage's query mask gates the
    pooled sums of every passage of the document (knrm).  Documents of 3 passages whose queries differ in length - shorter than A in
    the first passage, longer in the others and the other way round - against a transcription of knrm's lines on the per-passage
    matrices."""
    B, P, S, H, A, K = 4, 3, 32, 16, 6, 5
    g = torch.Generator().manual_seed(5)
    x = torch.randn((B * P, S, H), generator=g)
    qlens = [2, 9, 5, 8, 3, 4, 5, 5, 1, 4, 7, 2]            # tokens before [SEP]: rows 1..qlen+1 are query rows when they fit in A
    ms = [cedr_case.passage_masks(S, q, 10 + i) for i, q in enumerate(qlens)]
    mask, seg = (torch.from_numpy(np.stack([m[i] for m in ms])) for i in (0, 1))
    mask[4, 3] = 0                                           # a hole in a query row of a first passage and of a later one
    mask[7, 2] = 0
    mu, sigma = torch.tensor([-0.5, 0.0, 0.4, 0.9, 1.0]), torch.tensor([0.1, 0.3, 0.1, 0.1, 0.01])
    sim, dmask, own = cedr_case.ref_sims(x, mask, seg, A)
    assert not torch.equal(own.view(B, P, A)[:, 0], own.view(B, P, A)[:, 1])
    # knrm, CEDRKNRM_Class (passage_simmats / passage_doc_mask / passage_query_mask are what masked_simmats returned)
    passage_simmats = sim.view(B, P, A, S - 1)
    passage_doc_mask = dmask.view(B, P, 1, -1)
    doc_simmat = torch.cat([passage_simmats[:, PIDX, :, :] for PIDX in range(P)], dim=2)
    doc_mask = torch.cat([passage_doc_mask[:, PIDX, :, :] for PIDX in range(P)], dim=2)
    query_mask = own.view(B, P, -1, 1)[:, 0, :, :]
    prepooled_doc = torch.stack([torch.exp(-0.5 * (doc_simmat - m) ** 2 / s / s) for m, s in zip(mu.double(), sigma.double())], dim=1)
    prepooled_doc = prepooled_doc * doc_mask.view(B, 1, 1, -1) * query_mask.view(B, 1, -1, 1)
    want = prepooled_doc.sum(dim=3)                                                           # [B, K, A]
    qm0 = own.view(B, P, A)[:, 0].repeat_interleave(P, dim=0)
    got = cedr_case.ref_pk(x, mask, seg, qm0, A, mu, sigma)
    assert got.shape == (B * P, K, A)
    assert torch.allclose(got.view(B, P, K, A).sum(dim=1), want, rtol=1e-13, atol=1e-13)
    # the roles swapped, or the passage's own mask in both, is a different function on this case
    swapped = cedr_case.ref_pk(x, mask, seg, own, A, mu, sigma).view(B, P, K, A).sum(dim=1)
    assert (swapped - want).abs().max().item() > 1.0
    # and the document features that follow (clamp, log, sum over the query) through ref_score's kernel half
    w1 = torch.randn(K, generator=g)
    s, f = cedr_case.ref_score(got.unsqueeze(0), None, P, 0, w1, torch.zeros(1))
    feat = (torch.log(torch.clamp(want, min=1e-10)) * 0.01).sum(dim=2)
    assert torch.allclose(f, feat, rtol=1e-13, atol=1e-15) and torch.allclose(s, feat @ w1.double(), rtol=1e-12, atol=1e-15)
