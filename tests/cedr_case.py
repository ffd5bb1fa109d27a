"""CEDR-KNRM's similarity tap and document head restated in float64 torch (reference capreolus/reranker/CEDRKNRM.py:83-136, 160-185),
the chunk-major layout helpers, and seeded case builders for tests/test_gpu_cedr_tap.py.  tests/test_cedr_cpu.py pins the restatement
to oracle.bert_port.cedr_knrm and to the reference's recorded scores; it runs wherever its tensors live."""
import numpy as np
import torch

SUPPORTED_LENGTHS = (32, 64, 96, 128, 160, 192, 224, 256, 384, 512)
MAX_A, MAX_K = 32, 11


def to_cm(x):
    """row-major [M, C] -> the engine's chunk-major layout (include/capreolus_amd.h), flattened"""
    M, C = x.shape
    return x.reshape(M // 32, 32, C // 8, 8).permute(0, 2, 1, 3).contiguous().reshape(-1)


def from_cm(flat, M, C):
    return flat.reshape(M // 32, C // 8, 32, 8).permute(0, 2, 1, 3).contiguous().reshape(M, C)


def ln16(Pre, mr, gamma, beta, dtype):
    """The hidden state that pre-LayerNorm sums Pre [M, C] (16-bit) with row statistics mr [M, 2] = (mu, rstd) stand for: (float(P) - mu)
    * rstd in fp32 (two roundings), then ONE fused multiply-add with gamma / beta - the product of two fp32 values is exact in float64,
    so the float64 sum rounded to fp32 is the fma - rounded to the 16-bit type."""
    t = (Pre.float() - mr[:, :1].float()) * mr[:, 1:2].float()
    return (t.double() * gamma.double() + beta.double()).float().to(dtype)


def ref_sims(x, mask, seg, A, dtype=torch.float64):
    """masked_simmats / _cos_simmat (CEDRKNRM.py:84-107) on bert_output[:, 1:] (:111-113), in `dtype` arithmetic.
    x [np, S, H], mask / seg [np, S] -> (sim [np, A, S - 1], doc mask [np, S - 1], the passages' own query masks [np, A]); query rows at
    or beyond S - 1 are zero."""
    n, S, _ = x.shape
    emb, m, sg = x[:, 1:].to(dtype), mask[:, 1:].to(dtype), seg[:, 1:]
    qmask = m * (sg == 0).to(dtype)                                                           # :97
    q = (qmask.unsqueeze(2) * emb)[:, :A]                                                     # :98
    qmask = qmask[:, :A]                                                                      # :99
    dmask = m * (sg == 1).to(dtype)                                                           # :101
    d = dmask.unsqueeze(2) * emb                                                              # :103
    sim = q.bmm(d.transpose(1, 2)) / ((q.norm(p=2, dim=2).unsqueeze(2) + 1e-9) * (d.norm(p=2, dim=2).unsqueeze(1) + 1e-9))   # :88-90
    sim = sim * qmask.unsqueeze(2) * dmask.unsqueeze(1)                                       # :91-92
    if sim.shape[1] < A:
        sim = torch.cat([sim, sim.new_zeros(n, A - sim.shape[1], S - 1)], dim=1)
        qmask = torch.cat([qmask, qmask.new_zeros(n, A - qmask.shape[1])], dim=1)
    return sim, dmask, qmask


def ref_pk(x, mask, seg, qmask0, A, mu, sigma):
    """Per-passage kernel sums in the tap's layout [np][K][A], float64: the RBF kernels of the masked cosine matrix summed over the
    passage's document columns (:123-127), with qmask0 [np, A] - the query mask of the document's FIRST passage (:120), not the
    passage's own - applied to the sums."""
    sim, dmask, _ = ref_sims(x, mask, seg, A)
    mu = mu.double().view(1, -1, 1, 1)
    sg = sigma.double().view(1, -1, 1, 1)
    adj = sim.unsqueeze(1) - mu
    pre = torch.exp(-0.5 * adj * adj / sg / sg) * dmask.view(dmask.shape[0], 1, 1, -1) * qmask0.double().view(qmask0.shape[0], 1, A, 1)
    return pre.sum(dim=3)


def ref_score(pk, cls, P, cls_mode, w1, b1, w2=None, b2=None):
    """The document level (:114-133, 145-169) in float64.  pk [n_layers][B * P][K][A] (or None), cls [B * P][H] (or None), cls_mode
    0 none / 1 avg / 2 max; w1 [n_in] (single Linear) or [hidden, n_in] with w2 [hidden].  Returns (scores [B], features [B, n_in])."""
    feats = []
    if cls_mode:
        c = cls.double().view(-1, P, cls.shape[-1])
        feats.append(c.max(dim=1)[0] if cls_mode == 2 else c.mean(dim=1))
    if pk is not None and pk.shape[0] > 0:
        L, NP, K, A = pk.shape
        s = pk.double().view(L, NP // P, P, K, A).sum(dim=2)                                   # the passages side by side (:118)
        f = (torch.log(torch.clamp(s, min=1e-10)) * 0.01).sum(dim=3)                          # :128-131   [L, B, K]
        feats.append(f.permute(1, 0, 2).reshape(NP // P, L * K))
    x = torch.cat(feats, dim=1)
    if w2 is None:
        return x @ w1.double().view(-1) + b1.double().view(-1)[0], x
    h = x @ w1.double().t() + b1.double()
    return h @ w2.double().view(-1) + b2.double().view(-1)[0], x


# ---- case builders --------------------------------------------------------------------------------------------------------------

def passage_masks(S, qlen, dlen, doc_start=None):
    """[CLS] q_1 .. q_qlen [SEP] | d_1 .. d_dlen [SEP] | padding (mask 0, segment 0), as the extractor lays a passage out.  doc_start
    overrides the position of the first segment-1 token."""
    mask, seg = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    first = qlen + 2 if doc_start is None else doc_start
    end = min(S, first + dlen + 1)
    mask[:end] = 1
    seg[first:end] = 1
    return mask, seg


def make_case(S, H, A, K, n, p0=0, NP=None, seed=0, dtype=torch.float16, layout=0, device="cpu", sigmas=(0.1, 0.01, 0.3), zero_rows=(),
              qlens=None, unit_ln=False, masks=None):
    """A seeded tap call.  Hidden rows are N(offset_row, scale_row) (norms differ by row), every 7th document token is a copy of one
    of the passage's query tokens (similarity 1 up to rounding of the norms), rows listed in zero_rows [(passage, position)] are all
    zero.  layout 2 draws pre-LayerNorm sums, row statistics and gamma / beta, and the hidden state is ln16 of them (beta = 0 when
    there are zero rows: a zero hidden row then is a row equal to its mu); unit_ln: mu = 0, rstd = 1, gamma = 1, beta = 0.  masks: the
    passages' (mask, seg) rows instead of drawn ones.
    Returns a dict: x [n, S, H] the hidden state the reference reads; xin / mr / gamma / beta what the entry point is handed."""
    rs = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    NP = p0 + n if NP is None else NP
    raw = torch.randn((n, S, H), generator=g) * (0.25 + 1.75 * torch.rand((n, S, 1), generator=g)) + (torch.rand((n, S, 1), generator=g) - 0.5)
    mask, seg = np.zeros((n, S), dtype=np.int64), np.zeros((n, S), dtype=np.int64)
    for p in range(n):
        ql = int(rs.randint(1, A + 3)) if qlens is None else int(qlens[p % len(qlens)])
        ql = max(0, min(ql, S - 3))
        dl = int(rs.randint(1, S - ql - 2 + 1))
        if rs.rand() < 0.4:
            dl = S - ql - 3                                                # fills the passage: the last column is live
        mask[p], seg[p] = passage_masks(S, ql, max(dl, 0)) if masks is None else masks[p]
    copies = []
    for p in range(n):
        nq = int(((mask[p, 1:A + 1] != 0) & (seg[p, 1:A + 1] == 0)).sum())
        doc = np.nonzero(seg[p] == 1)[0]
        for j in doc[::7]:
            if nq:
                copies.append((p, int(j), 1 + int(rs.randint(0, nq))))
    stats = torch.stack([torch.rand((n * S,), generator=g) - 0.5, 0.5 + 1.5 * torch.rand((n * S,), generator=g)], dim=1)
    gamma, beta = 0.5 + torch.rand((H,), generator=g), 0.6 * torch.rand((H,), generator=g) - 0.3
    if zero_rows:
        beta = torch.zeros(H)
    if unit_ln:
        stats = torch.tensor([0.0, 1.0]).repeat(n * S, 1)
        gamma, beta = torch.ones(H), torch.zeros(H)
    raw16 = raw.to(dtype)
    stats = stats.view(n, S, 2).clone()
    for p, j, src in copies:
        raw16[p, j] = raw16[p, src]
        stats[p, j] = stats[p, src]
    for p, j in zero_rows:
        if layout == 2:
            raw16[p, j] = 0.25
            stats[p, j, 0] = 0.25
        else:
            raw16[p, j] = 0
    stats = stats.view(n * S, 2).contiguous()
    c = dict(S=S, H=H, A=A, K=K, n=n, p0=p0, NP=NP, layout=layout, dtype=dtype)
    if layout == 2:
        c["x"] = ln16(raw16.view(n * S, H), stats, gamma, beta, dtype).view(n, S, H)
        c["xin"], c["mr"], c["gamma"], c["beta"] = to_cm(raw16.view(n * S, H)), stats, gamma, beta
    else:
        c["x"] = raw16
        c["xin"] = to_cm(raw16.view(n * S, H)) if layout == 1 else raw16.reshape(-1).clone()
        c["mr"] = c["gamma"] = c["beta"] = None
    c["mask"], c["seg"] = torch.from_numpy(mask), torch.from_numpy(seg)
    c["qmask0"] = (torch.rand((NP, A), generator=g) < 0.8).float()
    c["mu"] = (2 * torch.rand((K,), generator=g) - 1).float()
    c["sigma"] = torch.tensor([sigmas[i] for i in rs.randint(0, len(sigmas), K)], dtype=torch.float32)
    for k in ("x", "xin", "mr", "gamma", "beta", "mask", "seg", "qmask0", "mu", "sigma"):
        if c[k] is not None:
            c[k] = c[k].to(device)
    return c


def cm_lds_bytes(S, H, A):
    """dynamic LDS of the chunk-major kernels (csrc/cedr_tap.h cedr_pool_cm_smem)"""
    return (4 * MAX_A + A * S + 2 * (MAX_K + 1) + 2 * MAX_A + S + 256 * (MAX_K + 1) + 2 * H) * 4 + H * 32 * 2
