"""Bags of words in CSR form, the input of the DSSM tower (capamd_dssm_tower, include/capreolus_amd.h).

The reference's BagOfWords extractor hands DSSM a dense [N, nvocab] count matrix (capreolus/extractor/bagofwords.py, transform_txt);
a document has a few hundred distinct terms at most, so the same rows are kept here as `indptr` int64 [N + 1], `idx` int32 [nnz] and
`val` fp32 [nnz], the entries of a row ordered by index.  This is format plumbing, not the hot path.
"""
from collections import namedtuple

import numpy as np
import torch


class Bags(namedtuple("Bags", ("indptr", "idx", "val"))):
    """(indptr int64 [N + 1], idx int32 [nnz], val fp32 [nnz]); bag n is the entries indptr[n] .. indptr[n + 1] - 1"""

    __slots__ = ()

    @property
    def rows(self):
        return int(self.indptr.shape[0]) - 1

    @property
    def device(self):
        return self.indptr.device

    def to(self, device, non_blocking=False):
        return Bags(*(t.to(device, non_blocking=non_blocking) for t in self))

    def to_dense(self, nvocab, dtype=torch.float32):
        """the [N, nvocab] matrix the reference reads (repeated indices of a bag add up)"""
        n = self.rows
        rows = torch.repeat_interleave(torch.arange(n, device=self.device), self.indptr[1:] - self.indptr[:-1])
        out = torch.zeros((n, nvocab), dtype=dtype, device=self.device)
        out.index_put_((rows, self.idx.long()), self.val.to(dtype), accumulate=True)
        return out


def from_dense(x):
    """a [N, nvocab] tensor -> Bags on x's device: its non-zero entries, each row's ordered by index"""
    if x.dim() != 2:
        raise ValueError(f"a bag-of-words matrix is [N, nvocab]; got shape {tuple(x.shape)}")
    nz = torch.nonzero(x)                                   # row-major: by row, then by index
    counts = torch.bincount(nz[:, 0], minlength=x.shape[0])
    indptr = torch.zeros(x.shape[0] + 1, dtype=torch.int64, device=x.device)
    indptr[1:] = torch.cumsum(counts, 0)
    return Bags(indptr, nz[:, 1].to(torch.int32), x[nz[:, 0], nz[:, 1]].to(torch.float32))


def from_term_ids(rows):
    """host side: a list of id arrays of any length -> Bags (CPU tensors) of unigram counts, sorted by id, as BagOfWords.transform_txt
    fills its vector (one count per occurrence)"""
    indptr, idx, val = [0], [], []
    for r in rows:
        ids, counts = np.unique(np.asarray(r, dtype=np.int64).reshape(-1), return_counts=True)
        idx.append(ids)
        val.append(counts)
        indptr.append(indptr[-1] + len(ids))
    cat = (lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt))
    return Bags(torch.from_numpy(np.asarray(indptr, dtype=np.int64)), torch.from_numpy(cat(idx, np.int32)), torch.from_numpy(cat(val, np.float32)))
