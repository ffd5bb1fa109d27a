"""The host side of DeepTileBar's colouring (reference capreolus/extractor/deeptileextractor.py): segment strings to ids and offsets,
the call into the colouring kernel, and a numpy statement of what that kernel computes.

Text tiling itself (nltk.TextTilingTokenizer, `extract_segment`) stays with the caller: this module takes its segments.

The reference colours a (query term, segment) tile from strings: `segment.split(" ")`, `segment_toks.count(q_tok)`,
`stoi.get(tok, pad)`.  On the device the same facts travel as ids:
  - a word `stoi` does not know gets id 0 and is looked up as the zero row, as `stoi.get(tok, 0)` does - it contributes
    exp(-|emb[q]|^2 / 2), not 0;
  - the literal pad token inside a segment gets id -1: the reference scores it as 0 and it can never equal a live query term;
  - a segment that IS the pad token (what `padlist` appends to short documents) becomes an empty range and so an all-zero tile;
  - an empty-string segment splits into one empty token, which `stoi` does not know: one token of id 0.
Two facts of the reference that callers meet: the extractor's `passagelen` overrides the reranker's, and `clean_segments` pads or
collapses to 30 segments whatever `passagelen` says, so only the first P of them are coloured.
"""
import numpy as np


def encode_segments(segments, stoi, pad_tok, P, L=None):
    """The first P of a document's segment strings -> (ids int64 [L], offsets int32 [P + 1]).  L: the row's length (None: as long as the
    tokens need); the row is filled up with 0 behind the last offset, where nothing is read."""
    if len(segments) < P:
        raise ValueError(f"{len(segments)} segments for P = {P} (clean_segments pads to 30)")
    ids, offsets = [], [0]
    for seg in segments[:P]:
        if seg != pad_tok:
            ids.extend(-1 if tok == pad_tok else stoi.get(tok, 0) for tok in seg.split(" "))
        offsets.append(len(ids))
    if L is None:
        L = max(len(ids), 1)
    if len(ids) > L:
        raise ValueError(f"the first {P} segments hold {len(ids)} tokens, more than L = {L}")
    row = np.zeros(L, dtype=np.int64)
    row[:len(ids)] = ids
    return row, np.asarray(offsets, dtype=np.int32)


def color(query, doc, seg_start, idf, emb, channels=3, check=True):
    """capamd_deeptile_color on device tensors: int64 query ids [B, Q] (pad 0), document ids [B, L], int32 offsets [B, P + 1], fp32 idf
    [B, Q], the fp32 table [V, D] -> fp32 tiles [B, Q, P, channels]"""
    from . import engine

    return engine.DeepTileEngine().color(query, doc, seg_start, idf, emb, channels, check=check)


def color_numpy(query, doc, seg_start, idf, emb, channels=3, dtype=np.float64):
    """What the colouring kernel computes, in numpy at `dtype` (ids in range, offsets non-decreasing inside the row): tiles
    [B, Q, P, channels]"""
    query, doc, seg_start = np.asarray(query), np.asarray(doc), np.asarray(seg_start)
    emb = np.asarray(emb).astype(dtype)
    B, Q = query.shape
    P = seg_start.shape[1] - 1
    out = np.zeros((B, Q, P, channels), dtype=dtype)
    for b in range(B):
        for p in range(P):
            toks = doc[b, seg_start[b, p]:seg_start[b, p + 1]]
            live = toks[toks >= 0]
            if not len(toks):
                continue
            for i in range(Q):
                q = query[b, i]
                if q == 0:
                    continue
                tf = int((live == q).sum())
                sim = np.exp(-((emb[live] - emb[q]) ** 2).sum(axis=1) / 2).max() if len(live) else 0.0
                out[b, i, p] = [tf, idf[b, i] if tf else 0.0, sim][3 - channels:]
    return out
