"""Thin PyTorch plumbing over the C-ABI library: device memory, streams, error surfacing.

PyTorch is used for exactly three things here: owning device buffers (caching allocator),
naming the current HIP stream, and holding the model parameters.  All arithmetic of the
scoring path happens inside libcapreolus_amd.so (capreolus_amd/csrc/*.hip).  There is no CPU
or eager-PyTorch fallback: inputs that are not on a HIP device raise.
"""
import ctypes
import math
import os

import threading

import torch

from . import _lib

HIST_TYPES = {"CH": 0, "NH": 1, "LCH": 2}
GATE_TYPES = {"IDF": 0, "TV": 1}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "capreolus_amd scores on an MI355X only: got a tensor on %s. There is no CPU fallback; "
                "move the batch and the model to 'cuda' (PytorchTrainer.predict does)." % t.device
            )


def _i64(t):
    return t if (t.dtype == torch.int64 and t.is_contiguous()) else t.to(torch.int64).contiguous()


def _f32(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


_deferred = [0]


class deferred_status:
    """Inside this context the per-call status read-backs (one 4-byte device->host copy, i.e. one synchronisation, per scoring
    call) are skipped; the bits keep accumulating in the device word and are raised when the context exits.  For callers that
    queue many scoring calls back to back (bench.py, a resident evaluation loop)."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    def __enter__(self):
        _deferred[0] += 1
        return self

    def __exit__(self, *exc):
        _deferred[0] -= 1
        if exc[0] is None and _deferred[0] == 0:
            status_word(self.device).raise_if_set()
        return False


class IdRangeError(IndexError, ValueError):
    """an id outside the embedding table: the IndexError nn.Embedding raises, and a ValueError as every other refused input is"""


class StatusWord:
    """The device int32 the kernels OR data-dependent error bits into (include/capreolus_amd.h)."""

    def __init__(self, device):
        self.t = torch.zeros(1, dtype=torch.int32, device=device)

    def raise_if_set(self):
        if _deferred[0]:
            return
        bits = int(self.t.item())  # synchronises, like the reference's .cpu() (trainer/pytorch.py:345)
        if bits:
            self.t.zero_()
            msgs = []
            if bits & _lib.STATUS_DOC_ID_RANGE:
                msgs.append("a document term id is outside the embedding table")
            if bits & _lib.STATUS_QUERY_ID_RANGE:
                msgs.append("a query term id is >= the embedding table size")
            if bits & _lib.STATUS_QUERY_OOV:
                msgs.append("a negative (OOV) query term id where the reference model cannot take one (DRMM.py:109, nn.Embedding in ConvKNRM.py:43)")
            if bits & _lib.STATUS_LIST_QUERY:
                raise ValueError("a candidate list holds pairs of more than one query (or idf row): a list is the pairs of ONE query, "
                                 "laid out as its offsets say (capamd_*_forward_lists)")
            if bits & (_lib.STATUS_SCORE_NAN | _lib.STATUS_TIE_RANGE):
                raise ValueError("ranking: " + ("a score is NaN; " if bits & _lib.STATUS_SCORE_NAN else "") +
                                 ("a tie-break rank is outside 0..n-1" if bits & _lib.STATUS_TIE_RANGE else ""))
            if bits & _lib.STATUS_SEGMENT_RANGE:
                raise ValueError("DeepTileBar colouring: a segment offset decreases or leaves [0, L] (it was clamped; nothing was read outside "
                                 "the row)")
            if bits & _lib.STATUS_BAG_RANGE:
                raise ValueError("DSSM: an indptr pair of the bags decreases or leaves [0, nnz] (it was clamped; nothing was read outside "
                                 "idx / val)")
            if bits & _lib.STATUS_SHORT_DOC:
                raise ValueError("POSITDRMM: a document has fewer than 2 non-pad terms (the reference's match statistics divide by its "
                                 "length and by its number of bigrams)")
            raise IdRangeError("index out of range in self: " + "; ".join(msgs))


_status_words = {}


def status_word(device):
    key = (device.type, device.index)
    if key not in _status_words:
        _status_words[key] = StatusWord(device)
    return _status_words[key]


_launch_hint = threading.local()


class concurrent_launches:
    """Context: the caller keeps several scoring calls in flight on different streams (the CAPAMD_LAUNCH_CONCURRENT flag of the
    interaction entries), e.g. one candidate list per launch round-robin over a few streams so that the tail of one list overlaps
    the next launch.  Per thread and nestable; the flag travels with each call, the library keeps no state."""

    def __enter__(self):
        _launch_hint.depth = getattr(_launch_hint, "depth", 0) + 1
        return self

    def __exit__(self, *exc):
        _launch_hint.depth -= 1
        return False


def _launch_flags():
    return _lib.LAUNCH_CONCURRENT if getattr(_launch_hint, "depth", 0) else 0


_workspaces = {}


def _workspace(device):
    """The few bytes of device memory an interaction call may use (capamd_interaction_workspace_bytes): one per (device, stream) -
    calls on one stream run in order, calls on different streams must not share it."""
    key = (device.index, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.zeros(max(16, int(_lib.load().capamd_interaction_workspace_bytes()) // 4), dtype=torch.int32, device=device)
    return ws


class PackedEmbedding:
    """The embedding table re-laid out for the gather kernels (capamd_pack_embeddings).

    Re-packed whenever the source weight changes (tracked with the tensor's version counter and
    storage pointer), so `load_weights` / fine-tuning never score against stale rows.
    """

    def __init__(self):
        self._key = None
        self.packed = None
        self.V = self.D = 0

    def get(self, weight):
        _need_gpu(weight)
        key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.device.index)
        if key != self._key:
            lib = _lib.load()
            w = _f32(weight.detach())
            V, D = w.shape
            nbytes = lib.capamd_packed_table_bytes(V, D)
            if nbytes < 0:
                raise ValueError(f"embedding dimension {D} is not supported by the packed layout (D <= 319)")
            packed = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            _lib.check(lib.capamd_pack_embeddings(_ptr(w), V, D, w.stride(0), _ptr(packed), _stream()), "capamd_pack_embeddings")
            self.packed, self.V, self.D, self._key = packed, V, D, key
        return self.packed


def similarity_matrix(query, doc, packed, V, D, check=True):
    """SimilarityMatrix.forward (reference common.py:170-182): fp32 [B, Q, L]."""
    _need_gpu(query, doc, packed)
    q, d = _i64(query), _i64(doc)
    B, Q = q.shape
    L = d.shape[1]
    out = torch.empty((B, Q, L), dtype=torch.float32, device=q.device)
    st = status_word(q.device)
    rc = _lib.load().capamd_similarity_matrix(_ptr(q), _ptr(d), B, Q, L, _ptr(packed), V, D, _ptr(out), _ptr(st.t), _stream())
    _lib.check(rc, "capamd_similarity_matrix")
    if check:
        st.raise_if_set()
    return out


def knrm_forward(query, doc, packed, V, D, mu, sigma, w1, b1, w2=None, b2=None, scoretanh=False, out=None, check=True):
    """KNRM_class.forward (reference KNRM.py:39-55): fp32 [B]."""
    _need_gpu(query, doc, packed, mu, sigma, w1, b1, w2, b2)
    q, d = _i64(query), _i64(doc)
    B, Q = q.shape
    L = d.shape[1]
    if d.shape[0] != B:
        raise AssertionError("query and document batch sizes differ")  # common.py:172
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=q.device)
    hidden = 0 if w2 is None else w1.shape[0]
    st, ws = status_word(q.device), _workspace(q.device)
    rc = _lib.load().capamd_knrm_forward(
        _ptr(q), _ptr(d), B, Q, L, _ptr(packed), V, D, _ptr(mu), _ptr(sigma), mu.numel(), _ptr(w1), _ptr(b1), hidden,
        _ptr(w2), _ptr(b2), int(bool(scoretanh)), _ptr(out), _ptr(st.t), _ptr(ws), ws.numel() * 4, _launch_flags(), _stream())
    _lib.check(rc, "capamd_knrm_forward")
    if check:
        st.raise_if_set()
    return out


def drmm_forward(query, doc, idf, packed, V, D, edges, hist_type, gate_type, gate_w, emb_raw, w1, b1, w2, b2, out_w, out_b,
                 out=None, counts_out=None, check=True):
    """DRMM_class.forward (reference DRMM.py:101-116): fp32 [B]."""
    _need_gpu(query, doc, idf, packed, edges, gate_w, w1, b1, w2, b2, out_w, out_b)
    q, d, idf = _i64(query), _i64(doc), _f32(idf)
    B, Q = q.shape
    L = d.shape[1]
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=q.device)
    st, ws = status_word(q.device), _workspace(q.device)
    ld = emb_raw.stride(0) if emb_raw is not None else 0
    rc = _lib.load().capamd_drmm_forward(
        _ptr(q), _ptr(d), _ptr(idf), B, Q, L, _ptr(packed), V, D, _ptr(edges), edges.numel(), HIST_TYPES[hist_type],
        GATE_TYPES[gate_type], _ptr(gate_w), _ptr(emb_raw), ld, _ptr(w1), _ptr(b1), w1.shape[0], _ptr(w2), _ptr(b2),
        _ptr(out_w), _ptr(out_b), _ptr(out), _ptr(counts_out), _ptr(st.t), _ptr(ws), ws.numel() * 4, _launch_flags(), _stream())
    _lib.check(rc, "capamd_drmm_forward")
    if check:
        st.raise_if_set()
    return out


AGGREGATIONS = {"max": 0, "first": 1, "sum": 2, "avg": 3}

_LAYER_TENSORS = (
    "attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight", "attention.self.key.bias",
    "attention.self.value.weight", "attention.self.value.bias", "attention.output.dense.weight", "attention.output.dense.bias",
    "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias",
    "output.dense.weight", "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias",
)


SUPPORTED_LENGTHS = tuple(range(32, 257, 32)) + (384, 512)   # the attention kernels of the library (capamd_bert_maxp_forward)


def _shorter_lengths(S, skip_padding, min_len=0):
    """the lengths above `min_len` a passage of S tokens may be encoded at instead (BertEngine._by_length)"""
    return [x for x in SUPPORTED_LENGTHS if min_len < x < S] if (skip_padding and S in SUPPORTED_LENGTHS) else []


class BertEngine:
    """Device-side state of one BERT sequence classifier for capamd_bert_maxp_forward.

    `params` maps the HF state_dict names (``bert.embeddings...``, ``bert.encoder.layer.N...``,
    ``bert.pooler.dense...``, ``classifier...``) to live fp32 parameters on the device.  The bf16
    weight blob is rebuilt whenever any parameter's version counter or storage changes.
    """

    COMPUTE_DTYPES = {"bf16": 0, "fp16": 1}

    def __init__(self, params, heads, microbatch=256, compute_dtype="fp16", skip_padding=True, ln_eps=0.0, pos_pad_id=-1):
        """ln_eps / pos_pad_id: RoBERTa bodies (include/capreolus_amd.h: capamd_bert_model) - LayerNorm epsilon (0 = BERT's 1e-12) and the
        padding id its position ids are counted around (-1 = BERT: position i)."""
        if compute_dtype not in self.COMPUTE_DTYPES:
            raise ValueError("compute_dtype must be 'bf16' or 'fp16'")
        self.ln_eps, self.pos_pad_id = float(ln_eps), int(pos_pad_id)
        self.params = params
        self.heads = heads
        self.microbatch = microbatch
        self.compute_dtype = compute_dtype
        self.skip_padding = skip_padding
        self._key = None
        self._blob = self._lf32 = None
        self._wss = {}        # workspaces: None -> the full-length call, Sb -> the length bucket running on its own stream
        self._streams = {}
        # the full-length path splits a large batch over this many HIP streams (own workspaces); 1 = strictly serial kernels
        self.n_streams = max(1, int(os.environ.get("CAPAMD_BERT_STREAMS", "2")))
        self._model = None
        self._keep = None

    def _dims(self):
        p = self.params
        hidden = p["bert.embeddings.word_embeddings.weight"].shape[1]
        layers = 1 + max(int(k.split(".")[3]) for k in p if k.startswith("bert.encoder.layer."))
        m = _lib.BertModel()
        m.hidden, m.layers, m.heads = hidden, layers, self.heads
        m.ffn = p["bert.encoder.layer.0.intermediate.dense.weight"].shape[0]
        m.vocab = p["bert.embeddings.word_embeddings.weight"].shape[0]
        m.max_pos = p["bert.embeddings.position_embeddings.weight"].shape[0]
        m.type_vocab = p["bert.embeddings.token_type_embeddings.weight"].shape[0]
        m.compute_dtype = self.COMPUTE_DTYPES[self.compute_dtype]
        m.ln_eps, m.pos_pad_id = self.ln_eps, self.pos_pad_id
        return m

    def model(self):
        p = self.params
        key = tuple((t.data_ptr(), t._version) for t in p.values()) + (self.compute_dtype,)
        if key == self._key:
            return self._model
        lib = _lib.load()
        some = p["bert.embeddings.word_embeddings.weight"]
        _need_gpu(*p.values())
        m = self._dims()
        nblob, nf = lib.capamd_bert_blob_bytes(ctypes.byref(m)), lib.capamd_bert_layer_f32_floats(ctypes.byref(m))
        if nblob < 0:
            raise ValueError("unsupported BERT geometry: need hidden == 64*heads, hidden % 64 == 0 (<= 1024), ffn % 64 == 0")
        blob = torch.empty(nblob, dtype=torch.uint8, device=some.device)
        lf32 = torch.empty(nf * m.layers, dtype=torch.float32, device=some.device)
        keep = {k: _f32(v.detach()) for k, v in p.items()}
        for layer in range(m.layers):
            ptrs = [keep[f"bert.encoder.layer.{layer}.{n}"].data_ptr() for n in _LAYER_TENSORS]
            # + the LayerNorm whose output feeds this layer (the previous layer's output LayerNorm; layer 0 reads the
            # already normalised embeddings): folded into this layer's QKV / O-proj epilogues (bert_gemm.h)
            prev = [keep[f"bert.encoder.layer.{layer - 1}.output.LayerNorm.{n}"].data_ptr() for n in ("weight", "bias")] if layer > 0 else [None, None]
            arr = (ctypes.c_void_p * 18)(*(ptrs + prev))
            _lib.check(lib.capamd_bert_pack_layer(ctypes.byref(m), layer, arr, _ptr(blob), _ptr(lf32), _stream()), "capamd_bert_pack_layer")
        for field, name in (("word_emb", "bert.embeddings.word_embeddings.weight"), ("pos_emb", "bert.embeddings.position_embeddings.weight"),
                            ("type_emb", "bert.embeddings.token_type_embeddings.weight"), ("emb_ln_g", "bert.embeddings.LayerNorm.weight"),
                            ("emb_ln_b", "bert.embeddings.LayerNorm.bias"), ("pooler_w", "bert.pooler.dense.weight"),
                            ("pooler_b", "bert.pooler.dense.bias"), ("cls_w", "classifier.weight"), ("cls_b", "classifier.bias")):
            # (pooler / classifier are absent for encoders that are only tapped - CEDR-KNRM on an ELECTRA body; capamd_bert_maxp_forward
            # refuses a model without them)
            setattr(m, field, keep[name].data_ptr() if name in keep else None)
        m.blob, m.layer_f32 = blob.data_ptr(), lf32.data_ptr()
        self._blob, self._lf32, self._keep, self._model, self._key = blob, lf32, keep, m, key
        return m

    def _workspace(self, key, S, n, device):
        """(model, workspace, micro-batch) of one encoder call over n passages of length S; `key` selects the workspace (one per
        concurrently running stream), which only ever grows."""
        m = self.model()
        # `microbatch` counts passages of 256 tokens: shorter passages go in proportionally larger micro-batches (same rows, same
        # workspace, and the GEMMs of a short-passage bucket still see 65,536 rows)
        mb = min(self.microbatch * max(1, 256 // S), n)
        need = _lib.load().capamd_bert_workspace_bytes(ctypes.byref(m), S, mb, n)
        if need < 0:
            raise ValueError(f"unsupported passage length {S} (supported: multiples of 32 up to 256, 384, 512)")
        ws = self._wss.get(key)
        if ws is None or ws.numel() < need or ws.device != device:
            ws = self._wss[key] = torch.empty(need, dtype=torch.uint8, device=device)
        return m, ws, mb

    def _side_stream(self, key, device):
        side = self._streams.get(key)
        if side is None:
            side = self._streams[key] = torch.cuda.Stream(device=device)
        return side

    def _by_length(self, ids, mask, seg, lengths, run, extras=(), outs=()):
        """Runs an encoder entry over the passages [NP, S] x3, each at the shortest of `lengths` (ascending, all < S; else S) that holds
        its last attended token.  `run(ids, mask, seg, S, extras, outs, ws_key)` makes the one library call on the current stream;
        `extras` are further per-passage inputs, `outs` (tensor, dim) pairs whose dimension `dim` counts the passages.  The buckets are
        independent: each runs on its own stream with its own workspace, so one bucket's kernels fill the CUs another bucket's last
        tiles leave idle and the launch gaps of one hide behind the work of the others.  Without `lengths`: one call on the caller's
        stream, writing straight into `outs`.  The caller has called model() on its stream: the (re)pack precedes the fan-out."""
        NP, S = ids.shape
        dev = ids.device
        if not lengths:
            run(ids, mask, seg, S, extras, [t for t, _ in outs], None)
            return
        # position after the last attended token of each passage (masks with holes keep their full extent)
        end = ((mask != 0) * torch.arange(1, S + 1, device=dev)).amax(dim=1)
        bounds = lengths + [S]
        bucket = torch.bucketize(end, torch.tensor(lengths, device=dev), right=False)   # 0: <= lengths[0], ...
        order = torch.argsort(bucket, stable=True)
        counts = torch.bincount(bucket, minlength=len(bounds)).cpu().tolist()   # the one host round trip of this call
        main = torch.cuda.current_stream(dev)
        lo, used = 0, []
        for Sb, n in zip(bounds, counts):
            if n == 0:
                continue
            sel = order[lo:lo + n]
            lo += n
            side = self._side_stream(Sb, dev)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                # (a ragged bucket is padded to whole 256-row GEMM tiles inside the library)
                bi, bm, bs = (t.index_select(0, sel)[:, :Sb].contiguous() for t in (ids, mask, seg))
                extras_b = [t.index_select(0, sel) for t in extras]
                outs_b = [torch.empty(t.shape[:dim] + (n,) + t.shape[dim + 1:], dtype=t.dtype, device=dev) for t, dim in outs]
                run(bi, bm, bs, Sb, extras_b, outs_b, Sb)
                for (t, dim), t_b in zip(outs, outs_b):
                    t.index_copy_(dim, sel, t_b)
                for t in (bi, bm, bs, *extras_b, *outs_b, sel):
                    t.record_stream(side)
            used.append(side)
        for side in used:
            main.wait_stream(side)

    def _encode(self, ids, mask, seg, B, P, S, aggregation, out, plog, check, ws_key=None):
        """One capamd_bert_maxp_forward call over [B, P, S] (all passages at length S) on the current stream."""
        m, ws, mb = self._workspace(ws_key, S, B * P, ids.device)
        st = status_word(ids.device)
        rc = _lib.load().capamd_bert_maxp_forward(_ptr(ids), _ptr(mask), _ptr(seg), B, P, S, ctypes.byref(m), AGGREGATIONS[aggregation], mb,
                                                  _ptr(ws), ws.numel(), _ptr(out), _ptr(plog), _ptr(st.t), _stream())
        _lib.check(rc, "capamd_bert_maxp_forward")
        if check:
            st.raise_if_set()

    def forward(self, doc_input, doc_mask, doc_seg, aggregation="max", return_passage_logits=False, check=True, skip_padding=None):
        """PTBERTMaxP_Class.predict_step (reference ptBERTMaxP.py:67-96): int64 [B,P,S] x3 -> fp32 [B].

        skip_padding (default: the engine's setting): encode every passage at the shortest supported length (SUPPORTED_LENGTHS) that
        holds its last attended token instead of at S.  Passages are independent, padded key positions get an attention
        weight of exactly 0 and padded query positions never reach the [CLS] row, so the passage logits are bit-identical to
        the full-length computation; only the dead rows are not computed.  Costs one small device->host copy (the bucket
        sizes) per call, like the reference's own `.cpu()` per batch."""
        _need_gpu(doc_input, doc_mask, doc_seg)
        if aggregation not in AGGREGATIONS:
            raise ValueError("Unknown aggregation method: {}".format(aggregation))
        ids, mask, seg = _i64(doc_input), _i64(doc_mask), _i64(doc_seg)
        B, P, S = ids.shape
        out = torch.empty(B, dtype=torch.float32, device=ids.device)
        if B == 0:
            return (out, torch.empty(0, device=ids.device)) if return_passage_logits else out
        if skip_padding is None:
            skip_padding = self.skip_padding
        if aggregation == "first" and not return_passage_logits and P > 1 and skip_padding:
            # ptBERTMaxP.py:85-86 takes scores[:, 0]: the other passages of a document are never read
            return self.forward(ids[:, :1], mask[:, :1], seg[:, :1], "first", False, check, skip_padding)
        NP = B * P
        fids, fmask, fseg = ids.view(NP, S), mask.view(NP, S), seg.view(NP, S)
        lengths = _shorter_lengths(S, skip_padding)
        if lengths:
            def run(bi, bm, bs, Sb, _, outs_b, ws_key):
                self._encode(bi, bm, bs, bi.shape[0], 1, Sb, "first", outs_b[0], None, False, ws_key=ws_key)

            plog = torch.empty(NP, dtype=torch.float32, device=ids.device)
            self.model()
            self._by_length(fids, fmask, fseg, lengths, run, outs=[(plog, 0)])
        else:
            q = 256 // math.gcd(S, 256)                      # passages per whole 256-row GEMM tile
            ns = max(1, min(self.n_streams, NP // self.microbatch))
            per = (NP // ns + q - 1) // q * q if ns > 1 else NP   # passages per stream, in whole tiles
            if ns > 1 and NP // ns >= 4 * self.microbatch and S == 256:
                # long runs: cut at whole micro-batches, so that every stream but the last runs FULL micro-batches only (whole rounds of
                # GEMM tiles on every CU, bert.hip: plan_microbatch) and one tail exists per call, not one per stream
                per = (NP // ns + self.microbatch - 1) // self.microbatch * self.microbatch
                if (ns - 1) * per >= NP:      # (five or more streams: rounding UP leaves the last stream nothing - round down instead)
                    per = NP // ns // self.microbatch * self.microbatch
            cuts = [min(NP, k * per) for k in range(ns)] + [NP]
            if ns < 2 or cuts[-2] >= NP:
                plog = torch.empty(NP, dtype=torch.float32, device=ids.device) if return_passage_logits else None
                self._encode(ids, mask, seg, B, P, S, aggregation, out, plog, check)
                return (out, plog) if return_passage_logits else out
            # full-length computation of a large batch: `ns` slices on as many streams (own workspaces) - the persistent GEMM kernels
            # of one slice start on the CUs the others' last tiles, low-occupancy kernels and launch gaps leave idle
            plog = torch.empty(NP, dtype=torch.float32, device=ids.device)
            self.model()
            main = torch.cuda.current_stream(ids.device)
            sides = []
            for k, (a0, a1) in enumerate(zip(cuts[:-1], cuts[1:])):
                side = self._side_stream(("half", k), ids.device)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    self._encode(fids[a0:a1], fmask[a0:a1], fseg[a0:a1], a1 - a0, 1, S, "first", plog[a0:a1], None, False, ws_key=("half", k))
                sides.append(side)
            for side in sides:
                main.wait_stream(side)
        if check:
            status_word(ids.device).raise_if_set()
        cnt = torch.empty(1, dtype=torch.int32, device=ids.device)
        _lib.check(_lib.load().capamd_maxp_pool(_ptr(plog), _ptr(mask), _ptr(seg), B, P, S, AGGREGATIONS[aggregation], _ptr(out), _ptr(cnt),
                                                _stream()), "capamd_maxp_pool")
        return (out, plog) if return_passage_logits else out


def _i32(t):
    return t if (t.dtype == torch.int32 and t.is_contiguous()) else t.to(torch.int32).contiguous()


def knrm_forward_indexed(q_table, d_table, pair_q, pair_d, packed, V, D, mu, sigma, w1, b1, w2=None, b2=None, scoretanh=False,
                         out=None, check=True):
    """KNRM over a device-resident candidate store (capamd_knrm_forward_indexed): int32 tables + per-pair rows."""
    _need_gpu(q_table, d_table, pair_q, pair_d, packed, mu, sigma, w1, b1, w2, b2)
    qt, dt, pq, pd = _i32(q_table), _i32(d_table), _i32(pair_q), _i32(pair_d)
    B, Q, L = pq.numel(), qt.shape[1], dt.shape[1]
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=pq.device)
    hidden = 0 if w2 is None else w1.shape[0]
    st, ws = status_word(pq.device), _workspace(pq.device)
    rc = _lib.load().capamd_knrm_forward_indexed(
        _ptr(qt), _ptr(dt), _ptr(pq), _ptr(pd), B, Q, L, _ptr(packed), V, D, _ptr(mu), _ptr(sigma), mu.numel(), _ptr(w1), _ptr(b1),
        hidden, _ptr(w2), _ptr(b2), int(bool(scoretanh)), _ptr(out), _ptr(st.t), _ptr(ws), ws.numel() * 4, _launch_flags(), _stream())
    _lib.check(rc, "capamd_knrm_forward_indexed")
    if check:
        st.raise_if_set()
    return out


def drmm_forward_indexed(q_table, d_table, idf_table, pair_q, pair_d, packed, V, D, edges, hist_type, gate_type, gate_w, emb_raw,
                         w1, b1, w2, b2, out_w, out_b, out=None, check=True):
    """DRMM over a device-resident candidate store (capamd_drmm_forward_indexed)."""
    _need_gpu(q_table, d_table, idf_table, pair_q, pair_d, packed, edges, gate_w, w1, b1, w2, b2, out_w, out_b)
    qt, dt, pq, pd, idf = _i32(q_table), _i32(d_table), _i32(pair_q), _i32(pair_d), _f32(idf_table)
    B, Q, L = pq.numel(), qt.shape[1], dt.shape[1]
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=pq.device)
    st, ws = status_word(pq.device), _workspace(pq.device)
    ld = emb_raw.stride(0) if emb_raw is not None else 0
    rc = _lib.load().capamd_drmm_forward_indexed(
        _ptr(qt), _ptr(dt), _ptr(idf), _ptr(pq), _ptr(pd), B, Q, L, _ptr(packed), V, D, _ptr(edges), edges.numel(),
        HIST_TYPES[hist_type], GATE_TYPES[gate_type], _ptr(gate_w), _ptr(emb_raw), ld, _ptr(w1), _ptr(b1), w1.shape[0], _ptr(w2),
        _ptr(b2), _ptr(out_w), _ptr(out_b), _ptr(out), None, _ptr(st.t), _ptr(ws), ws.numel() * 4, _launch_flags(), _stream())
    _lib.check(rc, "capamd_drmm_forward_indexed")
    if check:
        st.raise_if_set()
    return out


# ---- whole candidate lists (capamd_*_forward_lists) ------------------------------------------------------------------------------
_list_workspaces = {}
# Bytes the per-list part of a whole-list call's workspace may take (17 B x V per list in flight: 6.8 MB at V = 400,001, but 68 MB at
# V = 4 M - 64 lists would be 4.3 GB, the 256 a launch group takes 17 GB): fewer lists are kept in flight when it would be exceeded (the library then works through the
# lists in more, smaller groups).  The per-pair part (4 L + 32 bytes per pair of the call) comes on top.
LISTS_WORKSPACE_BUDGET = 2 << 30
LISTS_MAX_QLEN = 8          # query terms a whole-list call takes (csrc/lists.h: kListMaxQ; PACRR: 4)


def _lists_workspace(device, n_lists, nbytes_of, refusal):
    """The workspace of a whole-list call on the current stream, exactly as many bytes as the library asks for the lists kept in flight;
    `nbytes_of(k)`: what it asks for k of them (0: it does not take the geometry - ValueError(refusal))."""
    one = int(nbytes_of(1))
    if one == 0:
        raise ValueError(refusal)
    per_list = int(nbytes_of(2)) - one
    in_flight = max(1, min(int(n_lists), LISTS_WORKSPACE_BUDGET // max(per_list, 1)))
    nbytes = int(nbytes_of(in_flight))
    key = (device.index, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _list_workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _list_workspaces[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws[:nbytes]


def release_workspaces():
    """Drops the cached whole-list workspaces (one per device and stream; a later call allocates again)."""
    _list_workspaces.clear()


def _list_offsets(offsets):
    """host int64 array of n_lists + 1 pair offsets (kept alive by the caller's frame during the call)"""
    import numpy as np

    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64))
    if off.ndim != 1 or off.size < 1 or off[0] != 0 or (np.diff(off) < 0).any():
        raise ValueError("list offsets must start at 0 and be non-decreasing")
    return off


def _lists_ids(query, doc, store, pair_q, pair_d):
    """(q64, d64, q32, d32, pq, pd, B, Q, L, device): one of the two id layouts"""
    if store is not None:
        qt, dt, pq, pd = _i32(store.q_table), _i32(store.d_table), _i32(pair_q), _i32(pair_d)
        return None, None, qt, dt, pq, pd, pq.numel(), qt.shape[1], dt.shape[1], pq.device
    q, d = _i64(query), _i64(doc)
    return q, d, None, None, None, None, q.shape[0], q.shape[1], d.shape[1], q.device


def _lists_pair_workspace(device, n_lists, V, n_pairs, L, Q=4):
    """_lists_workspace of the entries of csrc/lists.hip (capamd_lists_workspace_bytes_q; n_pairs = 0: without the per-pair part)"""
    lib = _lib.load()
    return _lists_workspace(device, n_lists, lambda k: lib.capamd_lists_workspace_bytes_q(k, int(V), int(n_pairs), int(L), int(Q)),
                            f"whole-list scoring takes queries of up to {LISTS_MAX_QLEN} terms, got {Q}")


def _lists_call(offsets, query, doc, store, pair_q, pair_d, out, params):
    """What every whole-list wrapper starts with -> (the six id tensors of _lists_ids, host offsets, B, Q, L, device, out [B]);
    `params`: the call's other tensors, which must be on the device."""
    *ids, B, Q, L, dev = _lists_ids(query, doc, store, pair_q, pair_d)
    _need_gpu(*params)
    off = _list_offsets(offsets)
    if int(off[-1]) != B:
        raise ValueError("the last list offset must be the number of pairs")
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=dev)
    return ids, off, B, Q, L, dev, out


def knrm_forward_lists(offsets, packed, V, D, mu, sigma, w1, b1, w2=None, b2=None, scoretanh=False, query=None, doc=None, store=None, pair_q=None,
                       pair_d=None, out=None, check=True):
    """KNRM over whole candidate lists (capamd_knrm_forward_lists): pairs laid out list after list, `offsets` their n_lists + 1
    boundaries on the host; ids as [B, Q] / [B, L] tensors or through a CandidateStore (store, pair_q, pair_d)."""
    ids, off, B, Q, L, dev, out = _lists_call(offsets, query, doc, store, pair_q, pair_d, out, (packed, mu, sigma, w1, b1, w2, b2))
    hidden = 0 if w2 is None else w1.shape[0]
    st, ws = status_word(dev), _lists_pair_workspace(dev, off.size - 1, V, B, L, Q)
    rc = _lib.load().capamd_knrm_forward_lists(
        *map(_ptr, ids), ctypes.c_void_p(off.ctypes.data), off.size - 1, Q, L, _ptr(packed), V, D, _ptr(mu),
        _ptr(sigma), mu.numel(), _ptr(w1), _ptr(b1), hidden, _ptr(w2), _ptr(b2), int(bool(scoretanh)), _ptr(out), _ptr(st.t), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "capamd_knrm_forward_lists")
    if check:
        st.raise_if_set()
    return out


def drmm_forward_lists(offsets, idf, packed, V, D, edges, hist_type, gate_type, gate_w, emb_raw, w1, b1, w2, b2, out_w, out_b, query=None, doc=None,
                       store=None, pair_q=None, pair_d=None, out=None, counts_out=None, check=True):
    """DRMM over whole candidate lists (capamd_drmm_forward_lists); `idf`: [B, Q] per pair, or the store's [NQ, Q] table in indexed mode."""
    ids, off, B, Q, L, dev, out = _lists_call(offsets, query, doc, store, pair_q, pair_d, out, (packed, edges, gate_w, w1, b1, w2, b2, out_w, out_b))
    idf = _f32(idf)
    ld = emb_raw.stride(0) if emb_raw is not None else 0
    st, ws = status_word(dev), _lists_pair_workspace(dev, off.size - 1, V, B, L, Q)
    rc = _lib.load().capamd_drmm_forward_lists(
        *map(_ptr, ids), _ptr(idf), ctypes.c_void_p(off.ctypes.data), off.size - 1, Q, L, _ptr(packed), V, D,
        _ptr(edges), edges.numel(), HIST_TYPES[hist_type], GATE_TYPES[gate_type], _ptr(gate_w), _ptr(emb_raw), ld, _ptr(w1), _ptr(b1), w1.shape[0],
        _ptr(w2), _ptr(b2), _ptr(out_w), _ptr(out_b), _ptr(out), _ptr(counts_out), _ptr(st.t), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "capamd_drmm_forward_lists")
    if check:
        st.raise_if_set()
    return out


class AdamStep:
    """What a fused training step needs of a torch.optim.Adam: the parameters' device pointers with their moments (created the way
    Adam's own first step creates them), the host-side step count, and the step's scalars computed in double as the optimizer's
    non-capturable path does (torch/optim/adam.py: bias_correction = 1 - beta ** step; step_size = lr / bias_correction1;
    denom = sqrt(v) / sqrt(bias_correction2) + eps).  The state stays a plain Adam state_dict: checkpoints written during fused training
    load into the reference's trainer and vice versa."""

    def __init__(self, optimizer, params):
        if not isinstance(optimizer, torch.optim.Adam) or len(optimizer.param_groups) != 1:
            raise NotImplementedError("fused training steps follow torch.optim.Adam with one parameter group")
        g = optimizer.param_groups[0]
        if g.get("weight_decay", 0) or g.get("amsgrad") or g.get("maximize") or g.get("capturable") or torch.is_tensor(g["lr"]):
            raise NotImplementedError("fused training steps follow the plain Adam of the reference (no weight decay / amsgrad / capturable)")
        self.optimizer, self.group, self.params = optimizer, g, list(params)
        in_opt = {id(p) for p in g["params"]}
        # every tensor the optimizer trains must be one the device step updates: a parameter added to a model later would otherwise
        # silently never move under the fused step - on this error the trainer takes eager steps with the same optimizer
        missing = in_opt - {id(p) for p in self.params if p is not None}
        if missing:
            raise NotImplementedError(f"{len(missing)} optimizer parameter(s) are not covered by this reranker's device training step")
        ptrs = [[], [], []]
        for p in self.params:
            if p is None or id(p) not in in_opt:        # not trained (requires_grad False): no moments
                for col, v in zip(ptrs, (p.data_ptr() if p is not None else 0, 0, 0)):
                    col.append(v)
                continue
            st = optimizer.state[p]
            if len(st) == 0:       # (Adam._init_group)
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if st["step"].is_cuda:
                raise NotImplementedError("fused training steps keep Adam's step count on the host")
            for col, v in zip(ptrs, (p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr())):
                col.append(v)
        dev = next(p for p in self.params if p is not None).device
        self.table = torch.tensor(ptrs[0] + ptrs[1] + ptrs[2], dtype=torch.int64).to(dev)
        self.key = tuple(ptrs[0] + ptrs[1] + ptrs[2])
        self.trained = [p for p in self.params if p is not None and id(p) in in_opt]

    @classmethod
    def cached(cls, owner, optimizer, params):
        """The AdamStep `owner` (a model) keeps for `optimizer` - rebuilt when the optimizer, a parameter's storage or its moments changed."""
        hit = owner.__dict__.get("_adam_step")
        if hit is None or hit.optimizer is not optimizer or hit.key[: len(params)] != tuple(p.data_ptr() for p in params) or not hit.still_valid():
            hit = owner.__dict__["_adam_step"] = cls(optimizer, params)
        return hit

    def still_valid(self):
        st = self.optimizer.state
        return all(len(st[p]) and st[p]["exp_avg"].data_ptr() in self.key for p in self.trained)

    def advance(self):
        """(step_size, 1 - beta1, beta2, eps, sqrt(bias_correction2)) of the NEXT step.  The step counters move on in `commit()`, after
        the C call has validated its arguments and launched: an EngineError must not leave the count ahead of the moments."""
        b1, b2 = self.group["betas"]
        t = float(self.optimizer.state[self.trained[0]]["step"]) + 1.0
        return float(self.group["lr"]) / (1 - b1 ** t), 1 - b1, b2, float(self.group["eps"]), (1 - b2 ** t) ** 0.5

    def commit(self):
        for p in self.trained:
            self.optimizer.state[p]["step"] += 1


_step_workspaces = {}


def _train_step(entry, lead, ws_floats, adam, softmax, device, check):
    """The tail every capamd_*_train_step call shares: `lead` are the model's own leading arguments, then loss type, the Adam step's
    scalars, loss, workspace and status.  After a successful call the trained parameters' version counters are bumped (an exact no-op
    x * 1: the kernels wrote them behind autograd's back), so that weight-derived caches notice.  Returns the loss [1]."""
    ws = _step_workspace(device, int(ws_floats))
    loss = torch.empty(1, dtype=torch.float32, device=device)
    st = status_word(device)
    rc = getattr(_lib.load(), entry)(*lead, int(bool(softmax)), *adam.advance(), _ptr(loss), _ptr(ws), ws.numel(), _ptr(st.t), _stream())
    _lib.check(rc, entry)
    adam.commit()
    if check:
        st.raise_if_set()
    with torch.no_grad():
        torch._foreach_mul_(adam.trained, 1.0)
    return loss


def _host_table(adam):
    """The parameter / moment pointers as a host array (the entries whose kernels read them from launch arguments)."""
    return (ctypes.c_void_p * len(adam.key))(*[p or None for p in adam.key])


def knrm_train_step(query, posdoc, negdoc, packed, V, D, K, adam, train_kernels, scoretanh, softmax, check=True):
    """capamd_knrm_train_step: score(pos), score(neg), the trainer's pairwise loss, backward, Adam - on the device; returns the loss [1]."""
    _need_gpu(query, posdoc, negdoc, packed)
    q, dp, dn = _i64(query), _i64(posdoc), _i64(negdoc)
    B, Q = q.shape
    L = dp.shape[1]
    lead = (_ptr(q), _ptr(dp), _ptr(dn), B, Q, L, _ptr(packed), V, D, K, _ptr(adam.table), int(bool(train_kernels)), int(bool(scoretanh)))
    return _train_step("capamd_knrm_train_step", lead, _lib.load().capamd_knrm_train_step_workspace_floats(B, K), adam, softmax, q.device, check)


def convknrm_train_step(query, posdoc, negdoc, emb, G, F, K, crossmatch, adam, scoretanh, softmax, check=True):
    """capamd_convknrm_train_step: score(pos), score(neg), the trainer's pairwise loss, backward, Adam - on the device; returns the loss [1]."""
    _need_gpu(query, posdoc, negdoc, emb)
    q, dp, dn, e = _i64(query), _i64(posdoc), _i64(negdoc), _f32(emb.detach())
    B, Q = q.shape
    L = dp.shape[1]
    q2, d2 = torch.cat([q, q]), torch.cat([dp, dn])
    lead = (_ptr(q2), _ptr(d2), B, Q, L, _ptr(e), e.shape[0], e.shape[1], G, F, K, int(bool(crossmatch)), _host_table(adam), int(bool(scoretanh)))
    ws_floats = _lib.load().capamd_convknrm_train_step_workspace_floats(B, Q, L, e.shape[1], G, F, K, int(bool(crossmatch)))
    return _train_step("capamd_convknrm_train_step", lead, ws_floats, adam, softmax, q.device, check)


def pacrr_train_step_fits(B, Q, n_ngrams, kmax, use_idf, combine):
    """whether a batch's activations fit the one-workgroup stage of capamd_pacrr_train_step (include/capreolus_amd.h)"""
    H, X = int(combine), int(Q) * (int(n_ngrams) * int(kmax) + int(bool(use_idf)))
    return H <= 128 and H * X + H * H + H + 2 * B * X + 8 * B * H + 5 * B <= 36 * 1024


def pacrr_train_step(query, posdoc, negdoc, idf, packed, V, D, mingram, maxgram, nfilters, kmax, use_idf, combine, nonlinearity, adam, softmax, check=True):
    """capamd_pacrr_train_step: score(pos), score(neg), the trainer's pairwise loss, backward, Adam - on the device; returns the loss [1]."""
    _need_gpu(query, posdoc, negdoc, idf, packed)
    q, dp, dn, idf = _i64(query), _i64(posdoc), _i64(negdoc), _f32(idf)
    B, Q = q.shape
    L = dp.shape[1]
    q2, d2, idf2 = torch.cat([q, q]), torch.cat([dp, dn]), torch.cat([idf, idf])
    lead = (_ptr(q2), _ptr(d2), _ptr(idf2), B, Q, L, _ptr(packed), V, D, int(mingram), int(maxgram), int(nfilters), int(kmax), int(bool(use_idf)),
            int(combine), NONLINEARITIES[nonlinearity], _host_table(adam))
    ws_floats = _lib.load().capamd_pacrr_train_step_workspace_floats(B, Q, L, int(mingram), int(maxgram), int(nfilters), int(kmax))
    return _train_step("capamd_pacrr_train_step", lead, ws_floats, adam, softmax, q.device, check)


def _step_workspace(device, n):
    key = (device.index, int(torch.cuda.current_stream(device).cuda_stream))
    ws = _step_workspaces.get(key)
    if ws is None or ws.numel() < n:
        ws = _step_workspaces[key] = torch.empty(n, dtype=torch.float32, device=device)
    return ws


def drmm_train_step(query, posdoc, negdoc, idf, packed, V, D, edges, hist_type, nodes, adam, softmax, check=True):
    """capamd_drmm_train_step: score(pos), score(neg), the trainer's pairwise loss, backward, Adam - on the device; returns the loss [1]."""
    _need_gpu(query, posdoc, negdoc, idf, packed, edges)
    q, dp, dn, idf = _i64(query), _i64(posdoc), _i64(negdoc), _f32(idf)
    B, Q = q.shape
    L = dp.shape[1]
    lead = (_ptr(q), _ptr(dp), _ptr(dn), _ptr(idf), B, Q, L, _ptr(packed), V, D, _ptr(edges), edges.numel(), HIST_TYPES[hist_type], int(nodes),
            _ptr(adam.table))
    ws_floats = _lib.load().capamd_drmm_train_step_workspace_floats(B, Q, edges.numel(), int(nodes))
    return _train_step("capamd_drmm_train_step", lead, ws_floats, adam, softmax, q.device, check)


def drmmtks_train_step(query, posdoc, negdoc, idf, packed, V, D, topk, adam, softmax, check=True):
    """capamd_drmmtks_train_step: score(pos), score(neg), the trainer's pairwise loss, backward, Adam - on the device; returns the loss [1]."""
    _need_gpu(query, posdoc, negdoc, idf, packed)
    q, dp, dn, idf = _i64(query), _i64(posdoc), _i64(negdoc), _f32(idf)
    B, Q = q.shape
    L = dp.shape[1]
    lead = (_ptr(q), _ptr(dp), _ptr(dn), _ptr(idf), B, Q, L, _ptr(packed), V, D, int(topk), _ptr(adam.table))
    return _train_step("capamd_drmmtks_train_step", lead, _lib.load().capamd_drmmtks_train_step_workspace_floats(B, Q, int(topk)), adam, softmax,
                       q.device, check)


def knrm_features(query, doc, packed, V, D, mu, sigma, need_grad=True, check=True):
    """capamd_knrm_features: kernel-pooling features [B, K] and d f/d mu, d f/d sigma [B, K] (None when not needed)."""
    _need_gpu(query, doc, packed, mu, sigma)
    q, d = _i64(query), _i64(doc)
    B, Q = q.shape
    L, K = d.shape[1], mu.numel()
    feat = torch.empty((B, K), dtype=torch.float32, device=q.device)
    dmu = torch.empty_like(feat) if need_grad else None
    dsg = torch.empty_like(feat) if need_grad else None
    st = status_word(q.device)
    rc = _lib.load().capamd_knrm_features(_ptr(q), _ptr(d), B, Q, L, _ptr(packed), V, D, _ptr(mu), _ptr(sigma), K, _ptr(feat),
                                          _ptr(dmu), _ptr(dsg), _ptr(st.t), _stream())
    _lib.check(rc, "capamd_knrm_features")
    if check:
        st.raise_if_set()
    return feat, dmu, dsg


class KnrmFeatures(torch.autograd.Function):
    """features = f(query, doc; mu, sigma) with the HIP kernel supplying both the value and the two Jacobian diagonals
    (f_k depends on mu_k / sigma_k only), so `combine` and the loss can sit on top of it under autograd."""

    @staticmethod
    def forward(ctx, mu, sigma, query, doc, packed, V, D):
        need = mu.requires_grad or sigma.requires_grad
        feat, dmu, dsg = knrm_features(query, doc, packed, V, D, mu.detach().float().contiguous(), sigma.detach().float().contiguous(),
                                       need_grad=need)
        if need:
            ctx.save_for_backward(dmu, dsg)
        ctx.has = need
        return feat

    @staticmethod
    def backward(ctx, g):
        if not ctx.has:
            return (None,) * 7
        dmu, dsg = ctx.saved_tensors
        return (g * dmu).sum(0), (g * dsg).sum(0), None, None, None, None, None


def similarity_matrix_autograd(embedding, query, doc):
    """SimilarityMatrix.forward (capreolus/reranker/common.py:155-182) as ATen ops under autograd ON THE GPU, for the configurations in
    which the embedding table trains (KNRM finetune=True, DRMM-TKS freezeemb=False): the gradient has to reach the [V, D] table through
    both operands of every cosine, which the HIP front end (frozen tables only) does not provide.  Exact matches of OOV terms (negative
    ids) + cosine of in-vocabulary terms (everything else looks up row 0), pads zeroed.  -> [B, Q, L]."""
    _need_gpu(query, doc, embedding.weight)
    q, d = query.long(), doc.long()
    qo, do = q.clamp(max=0), d.clamp(max=0)
    exact = (qo[:, :, None] == do[:, None, :]).float().masked_fill((qo == 0)[:, :, None], 0.0).masked_fill((do == 0)[:, None, :], 0.0)
    qi, di = q.clamp(min=0), d.clamp(min=0)
    a, b = embedding(qi), embedding(di)
    den = (a.norm(p=2, dim=2)[:, :, None] + 1e-9) * (b.norm(p=2, dim=2)[:, None, :] + 1e-9)
    cos = (a.bmm(b.permute(0, 2, 1)) / den).masked_fill((qi == 0)[:, :, None], 0.0).masked_fill((di == 0)[:, None, :], 0.0)
    return exact + cos


class NgramConv(torch.autograd.Function):
    """ConvKNRM's n-gram convolutions over the frozen embedding table, differentiable in their weights and biases
    (capamd_ngram_conv_forward / _backward; ConvKNRM.py:42-51 under the trainer's loss.backward()).
    apply(q_ids [N, Q], d_ids [N, L], emb [V, D], w_1, b_1, ..., w_G, b_G) -> qrep [N, G, Q, F], drep [N, G, L, F]."""

    @staticmethod
    def forward(ctx, q_ids, d_ids, emb, *wb):
        _need_gpu(q_ids, d_ids, emb, *wb)
        qi, di, e = _i64(q_ids), _i64(d_ids), _f32(emb.detach())
        ws, bs = [_f32(w.detach()) for w in wb[0::2]], [_f32(b.detach()) for b in wb[1::2]]
        G, F, D = len(ws), ws[0].shape[0], e.shape[1]
        N, Q, L = qi.shape[0], qi.shape[1], di.shape[1]
        lib = _lib.load()
        qrep = torch.empty((N, G, Q, F), dtype=torch.float32, device=e.device)
        drep = torch.empty((N, G, L, F), dtype=torch.float32, device=e.device)
        work = _step_workspace(e.device, int(lib.capamd_ngram_conv_workspace_floats(D, G, F, 0)))
        wp, bp = (ctypes.c_void_p * G)(*[w.data_ptr() for w in ws]), (ctypes.c_void_p * G)(*[b.data_ptr() for b in bs])
        st = status_word(e.device)
        rc = lib.capamd_ngram_conv_forward(_ptr(qi), _ptr(di), N, Q, L, _ptr(e), e.shape[0], D, wp, bp, G, F, _ptr(qrep), _ptr(drep), _ptr(work),
                                           work.numel(), _ptr(st.t), _stream())
        _lib.check(rc, "capamd_ngram_conv_forward")
        st.raise_if_set()
        ctx.save_for_backward(qi, di, e)
        ctx.geom = (G, F, [tuple(w.shape) for w in ws])
        return qrep, drep

    @staticmethod
    def backward(ctx, dq, dd):
        qi, di, e = ctx.saved_tensors
        G, F, shapes = ctx.geom
        N, Q, L, D = qi.shape[0], qi.shape[1], di.shape[1], e.shape[1]
        lib = _lib.load()
        dws = [torch.empty(sh, dtype=torch.float32, device=e.device) for sh in shapes]
        dbs = [torch.empty(F, dtype=torch.float32, device=e.device) for _ in shapes]
        work = _step_workspace(e.device, int(lib.capamd_ngram_conv_workspace_floats(D, G, F, 1)))
        wp, bp = (ctypes.c_void_p * G)(*[w.data_ptr() for w in dws]), (ctypes.c_void_p * G)(*[b.data_ptr() for b in dbs])
        dq, dd = _f32(dq), _f32(dd)
        st = status_word(e.device)
        rc = lib.capamd_ngram_conv_backward(_ptr(qi), _ptr(di), N, Q, L, _ptr(e), e.shape[0], D, G, F, _ptr(dq), _ptr(dd), wp, bp, _ptr(work),
                                            work.numel(), _ptr(st.t), _stream())
        _lib.check(rc, "capamd_ngram_conv_backward")
        out = [None, None, None]
        for w, b in zip(dws, dbs):
            out += [w, b]
        return tuple(out)


class KernelPool(torch.autograd.Function):
    """Cosine similarity + RBF kernel pooling over dense n-gram views, differentiable in both operands and in (mu, sigma)
    (capamd_kernel_pool_forward / _backward): ConvKNRM's training step between its convolutions and `combine`.
    qrep [B, GQ, Q, F], drep [B, GD, L, F] -> features [B, K V] in the reference's order (ConvKNRM.py:66-75)."""

    @staticmethod
    def forward(ctx, qrep, drep, q_ids, d_ids, mu, sigma, crossmatch):
        _need_gpu(qrep, drep, q_ids, d_ids, mu, sigma)
        qr, dr, qi, di = _f32(qrep.detach()), _f32(drep.detach()), _i64(q_ids), _i64(d_ids)
        m, sg = _f32(mu.detach()), _f32(sigma.detach())
        B, GQ, Q, F = qr.shape
        GD, L = dr.shape[1], dr.shape[2]
        K = m.numel()
        V = GQ * GD if crossmatch else GD
        T = (GQ if crossmatch else 1) * Q
        feat = torch.empty((B, K * V), dtype=torch.float32, device=qr.device)
        ksum = torch.empty((B, GD, T, K), dtype=torch.float32, device=qr.device)
        rowsum = torch.empty((B, GD, T), dtype=torch.float32, device=qr.device)
        C = int(_lib.load().capamd_kernel_pool_chunks(L))
        sums = torch.empty((B, GD, C, T, K + 1), dtype=torch.float32, device=qr.device)
        rc = _lib.load().capamd_kernel_pool_forward(_ptr(qr), _ptr(dr), _ptr(qi), _ptr(di), B, GQ, GD, Q, L, F, int(bool(crossmatch)), _ptr(m), _ptr(sg), K,
                                                    _ptr(feat), _ptr(ksum), _ptr(rowsum), _ptr(sums), _stream())
        _lib.check(rc, "capamd_kernel_pool_forward")
        ctx.save_for_backward(qr, dr, qi, di, m, sg, ksum, rowsum)
        ctx.crossmatch = bool(crossmatch)
        return feat

    @staticmethod
    def backward(ctx, g):
        qr, dr, qi, di, m, sg, ksum, rowsum = ctx.saved_tensors
        B, GQ, Q, F = qr.shape
        GD, L = dr.shape[1], dr.shape[2]
        K, T = m.numel(), ksum.shape[2]
        C = int(_lib.load().capamd_kernel_pool_chunks(L))
        dq_part = torch.empty((B, GD, C, T, F), dtype=torch.float32, device=qr.device)
        dd = torch.empty_like(dr)
        dmu = torch.empty((B * GD * C, K), dtype=torch.float32, device=qr.device)
        dsg = torch.empty_like(dmu)
        rc = _lib.load().capamd_kernel_pool_backward(_ptr(qr), _ptr(dr), _ptr(qi), _ptr(di), B, GQ, GD, Q, L, F, int(ctx.crossmatch), _ptr(m), _ptr(sg), K,
                                                     _ptr(_f32(g)), _ptr(ksum), _ptr(rowsum), _ptr(dq_part), _ptr(dd), _ptr(dmu), _ptr(dsg), _stream())
        _lib.check(rc, "capamd_kernel_pool_backward")
        # (without crossmatch block gd holds query view gd: T = Q)
        dq = dq_part.view(B, GD * C, GQ, Q, F).sum(1) if ctx.crossmatch else dq_part.sum(2)
        return dq, dd, None, None, dmu.sum(0), dsg.sum(0), None


class PacrrConvMax(torch.autograd.Function):
    """PACRR's n-gram Conv2d -> ReLU -> max over filters -> k-max over the document on a [B, Q, L] similarity matrix, with the
    gradient into the convolution weights (capamd_pacrr_convmax_forward / _backward; PACRR.py:68-78).  No gradient into `sim`:
    the embedding table behind it is frozen (PACRR.py:26)."""

    @staticmethod
    def forward(ctx, sim, conv_w, conv_b, mingram, maxgram, nfilters, kmax):
        _need_gpu(sim, conv_w, conv_b)
        x, w, b = _f32(sim.detach()), _f32(conv_w.detach()), _f32(conv_b.detach())
        B, Q, L = x.shape
        n = (maxgram - mingram + 1) * kmax
        top = torch.empty((B, Q, n), dtype=torch.float32, device=x.device)
        pos = torch.empty((B, Q, n), dtype=torch.int32, device=x.device)
        filt = torch.empty_like(pos)
        rc = _lib.load().capamd_pacrr_convmax_forward(_ptr(x), B, Q, L, mingram, maxgram, nfilters, kmax, _ptr(w), _ptr(b), _ptr(top), _ptr(pos), _ptr(filt),
                                                      _stream())
        _lib.check(rc, "capamd_pacrr_convmax_forward")
        ctx.save_for_backward(x, pos, filt)
        ctx.geom = (mingram, maxgram, nfilters, kmax, w.numel(), b.numel())
        return top

    @staticmethod
    def backward(ctx, g):
        x, pos, filt = ctx.saved_tensors
        mingram, maxgram, nfilters, kmax, nw, nb = ctx.geom
        B, Q, L = x.shape
        dw = torch.empty(nw, dtype=torch.float32, device=x.device)
        db = torch.empty(nb, dtype=torch.float32, device=x.device)
        rc = _lib.load().capamd_pacrr_convmax_backward(_ptr(x), B, Q, L, mingram, maxgram, nfilters, kmax, _ptr(_f32(g)), _ptr(pos), _ptr(filt), _ptr(dw),
                                                       _ptr(db), _stream())
        _lib.check(rc, "capamd_pacrr_convmax_backward")
        return None, dw, db, None, None, None, None


def drmm_features(query, doc, packed, V, D, edges, hist_type, check=True):
    """capamd_drmm_features: matching-histogram features [B, Q, nbins+1] (no trainable inputs)."""
    _need_gpu(query, doc, packed, edges)
    q, d = _i64(query), _i64(doc)
    B, Q = q.shape
    feat = torch.empty((B, Q, edges.numel() + 1), dtype=torch.float32, device=q.device)
    st = status_word(q.device)
    rc = _lib.load().capamd_drmm_features(_ptr(q), _ptr(d), B, Q, d.shape[1], _ptr(packed), V, D, _ptr(edges), edges.numel(),
                                          HIST_TYPES[hist_type], _ptr(feat), _ptr(st.t), _stream())
    _lib.check(rc, "capamd_drmm_features")
    if check:
        st.raise_if_set()
    return feat


def drmmtks_forward(query, doc, idf, packed, V, D, topk, gate_w, ffw_w, ffw_b, out_w, out_b, out=None, check=True):
    """DRMMTKS_class.forward (reference DRMMTKS.py:50-64): fp32 [B]."""
    _need_gpu(query, doc, idf, packed, gate_w, ffw_w, ffw_b, out_w, out_b)
    q, d, idf = _i64(query), _i64(doc), _f32(idf)
    B, Q = q.shape
    L = d.shape[1]
    if topk > L:
        raise RuntimeError("selected index k out of range")  # what torch.topk raises at DRMMTKS.py:56
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=q.device)
    st = status_word(q.device)
    rc = _lib.load().capamd_drmmtks_forward(_ptr(q), _ptr(d), _ptr(idf), B, Q, L, _ptr(packed), V, D, int(topk), _ptr(gate_w), _ptr(ffw_w),
                                            _ptr(ffw_b), _ptr(out_w), _ptr(out_b), _ptr(out), _ptr(st.t), _stream())
    _lib.check(rc, "capamd_drmmtks_forward")
    if check:
        st.raise_if_set()
    return out


def drmmtks_forward_lists(offsets, idf, packed, V, D, topk, gate_w, ffw_w, ffw_b, out_w, out_b, query=None, doc=None, store=None, pair_q=None,
                          pair_d=None, out=None, check=True):
    """DRMM-TKS over whole candidate lists (capamd_drmmtks_forward_lists); `idf`: [B, Q] per pair, or the store's [NQ, Q] table."""
    ids, off, B, Q, L, dev, out = _lists_call(offsets, query, doc, store, pair_q, pair_d, out, (packed, gate_w, ffw_w, ffw_b, out_w, out_b))
    if topk > L:
        raise RuntimeError("selected index k out of range")  # what torch.topk raises at DRMMTKS.py:56
    idf = _f32(idf)
    st, ws = status_word(dev), _lists_pair_workspace(dev, off.size - 1, V, B, L, Q)
    rc = _lib.load().capamd_drmmtks_forward_lists(
        *map(_ptr, ids), _ptr(idf), ctypes.c_void_p(off.ctypes.data), off.size - 1, Q, L, _ptr(packed), V, D,
        int(topk), _ptr(gate_w), _ptr(ffw_w), _ptr(ffw_b), _ptr(out_w), _ptr(out_b), _ptr(out), _ptr(st.t), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "capamd_drmmtks_forward_lists")
    if check:
        st.raise_if_set()
    return out


def drmmtks_features(query, doc, packed, V, D, topk, check=True):
    """The sorted top-k similarities of every query term (DRMMTKS.py:55-56): fp32 [B, Q, topk] (capamd_drmmtks_features)."""
    _need_gpu(query, doc, packed)
    q, d = _i64(query), _i64(doc)
    B, Q = q.shape
    L = d.shape[1]
    if topk > L:
        raise RuntimeError("selected index k out of range")
    out = torch.empty((B, Q, topk), dtype=torch.float32, device=q.device)
    st = status_word(q.device)
    rc = _lib.load().capamd_drmmtks_features(_ptr(q), _ptr(d), B, Q, L, _ptr(packed), V, D, int(topk), _ptr(out), _ptr(st.t), _stream())
    _lib.check(rc, "capamd_drmmtks_features")
    if check:
        st.raise_if_set()
    return out


NONLINEARITIES = {"none": 0, "relu": 1, "tanh": 2}


def pacrr_forward(query, doc, idf, packed, V, D, mingram, maxgram, nfilters, kmax, conv_w, conv_b, use_idf, nonlinearity, w1, b1, w2, b2,
                  w3, b3, out=None, check=True):
    """PACRR_class.forward (reference PACRR.py:42-55): fp32 [B].  conv_w / conv_b: the n-gram modules' Conv2d weights /
    biases, flattened back to back (capamd_pacrr_forward)."""
    _need_gpu(query, doc, idf, packed, conv_w, conv_b, w1, b1, w2, b2, w3, b3)
    q, d, idf = _i64(query), _i64(doc), _f32(idf)
    B, Q = q.shape
    L = d.shape[1]
    if kmax > L:
        raise RuntimeError("selected index k out of range")  # what torch.topk raises at PACRR.py:74
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=q.device)
    st = status_word(q.device)
    rc = _lib.load().capamd_pacrr_forward(_ptr(q), _ptr(d), _ptr(idf), B, Q, L, _ptr(packed), V, D, int(mingram), int(maxgram), int(nfilters),
                                          int(kmax), _ptr(conv_w), _ptr(conv_b), int(bool(use_idf)), w1.shape[0], NONLINEARITIES[nonlinearity],
                                          _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(out), _ptr(st.t), _stream())
    _lib.check(rc, "capamd_pacrr_forward")
    if check:
        st.raise_if_set()
    return out


def pacrr_forward_lists(offsets, idf, packed, V, D, mingram, maxgram, nfilters, kmax, conv_w, conv_b, use_idf, nonlinearity, w1, b1, w2, b2, w3, b3,
                        query=None, doc=None, store=None, pair_q=None, pair_d=None, out=None, check=True, pair_part=True):
    """PACRR over whole candidate lists (capamd_pacrr_forward_lists); `idf`: [B, Q] per pair, or the store's [NQ, Q] table.
    `pair_part=False` hands the library a workspace without the per-pair part (capamd_lists_workspace_bytes with n_pairs = 0): the combine
    layers then run at the end of every pair's convolution workgroup instead of in one pass behind them - the same scores, bit for bit."""
    ids, off, B, Q, L, dev, out = _lists_call(offsets, query, doc, store, pair_q, pair_d, out, (packed, conv_w, conv_b, w1, b1, w2, b2, w3, b3))
    if kmax > L:
        raise RuntimeError("selected index k out of range")  # what torch.topk raises at PACRR.py:74
    idf = _f32(idf)
    st, ws = status_word(dev), _lists_pair_workspace(dev, off.size - 1, V, B if pair_part else 0, L)
    rc = _lib.load().capamd_pacrr_forward_lists(
        *map(_ptr, ids), _ptr(idf), ctypes.c_void_p(off.ctypes.data), off.size - 1, Q, L, _ptr(packed), V, D,
        int(mingram), int(maxgram), int(nfilters), int(kmax), _ptr(conv_w), _ptr(conv_b), int(bool(use_idf)), w1.shape[0], NONLINEARITIES[nonlinearity],
        _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(w3), _ptr(b3), _ptr(out), _ptr(st.t), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "capamd_pacrr_forward_lists")
    if check:
        st.raise_if_set()
    return out


class ConvProjectionTables:
    """ConvKNRM's Conv1d layers folded into per-token projection tables (capamd_convknrm_pack_tables).  Rebuilt whenever the
    embedding table or any convolution parameter changes (version counters + storage pointers)."""

    def __init__(self):
        self._key = None
        self.tables = None

    def get(self, weight, conv_ws, conv_bs):
        _need_gpu(weight, *conv_ws, *conv_bs)
        key = tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in (weight, *conv_ws, *conv_bs)) + (weight.device.index,)
        if key != self._key:
            lib = _lib.load()
            w = _f32(weight.detach())
            V, D = w.shape
            G, F = len(conv_ws), conv_ws[0].shape[0]
            nbytes = lib.capamd_convknrm_table_bytes(V, G, F)
            if nbytes < 0:
                raise ValueError(f"ConvKNRM geometry maxngram={G}, filters={F} is not supported (maxngram <= 3, filters a multiple of 16 up to 128)")
            cw = torch.cat([_f32(c.detach()).reshape(-1) for c in conv_ws]).contiguous()
            cb = torch.cat([_f32(c.detach()).reshape(-1) for c in conv_bs]).contiguous()
            tables = torch.empty(nbytes // 4, dtype=torch.float32, device=w.device)
            _lib.check(lib.capamd_convknrm_pack_tables(_ptr(w), V, D, w.stride(0), _ptr(cw), _ptr(cb), G, F, _ptr(tables), _stream()),
                       "capamd_convknrm_pack_tables")
            self.tables, self._key = tables, key
        return self.tables


def convknrm_forward(query, doc, tables, V, maxngram, filters, crossmatch, mu, sigma, w1, b1, w2=None, b2=None, score_tanh=False, out=None,
                     check=True):
    """ConvKNRM_class.forward (reference ConvKNRM.py:42-77): fp32 [B].  w2 is None: single combine layer."""
    _need_gpu(query, doc, tables, mu, sigma, w1, b1)
    q, d = _i64(query), _i64(doc)
    B, Q = q.shape
    L = d.shape[1]
    if out is None:
        out = torch.empty(B, dtype=torch.float32, device=q.device)
    st = status_word(q.device)
    H = 0 if w2 is None else w1.shape[0]
    rc = _lib.load().capamd_convknrm_forward(_ptr(q), _ptr(d), B, Q, L, _ptr(tables), V, int(maxngram), int(filters), int(bool(crossmatch)),
                                             _ptr(mu), _ptr(sigma), mu.numel(), _ptr(w1), _ptr(b1), H, None if w2 is None else _ptr(w2),
                                             None if b2 is None else _ptr(b2), int(bool(score_tanh)), _ptr(out), _ptr(st.t), _stream())
    _lib.check(rc, "capamd_convknrm_forward")
    if check:
        st.raise_if_set()
    return out


def convknrm_forward_lists(offsets, query, doc, tables, V, maxngram, filters, crossmatch, mu, sigma, w1, b1, w2=None, b2=None, score_tanh=False, out=None,
                           check=True):
    """ConvKNRM over whole candidate lists (capamd_convknrm_forward_lists): pairs laid out list after list, `offsets` their n_lists + 1
    boundaries on the host; the unigram document view once per distinct token of a list.  Scores equal convknrm_forward's bit for bit."""
    (q, d, *_), off, B, Q, L, dev, out = _lists_call(offsets, query, doc, None, None, None, out, (query, doc, tables, mu, sigma, w1, b1))
    lib = _lib.load()
    ws = _lists_workspace(dev, off.size - 1, lambda k: lib.capamd_convknrm_lists_workspace_bytes(k, int(V), Q, int(maxngram), int(filters)),
                          "capamd_convknrm_forward_lists does not take this geometry")
    st = status_word(dev)
    H = 0 if w2 is None else w1.shape[0]
    rc = lib.capamd_convknrm_forward_lists(_ptr(q), _ptr(d), ctypes.c_void_p(off.ctypes.data), off.size - 1, Q, L, _ptr(tables), V, int(maxngram), int(filters),
                                           int(bool(crossmatch)), _ptr(mu), _ptr(sigma), mu.numel(), _ptr(w1), _ptr(b1), H,
                                           None if w2 is None else _ptr(w2), None if b2 is None else _ptr(b2), int(bool(score_tanh)), _ptr(out),
                                           _ptr(st.t), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "capamd_convknrm_forward_lists")
    if check:
        st.raise_if_set()
    return out


CLS_MODES = {None: 0, "avg": 1, "max": 2}


class CedrEngine:
    """CEDR-KNRM on top of a BertEngine's packed encoder: capamd_cedr_passage_features (encoder + per-layer masked cosine matrices +
    kernel pooling) followed by capamd_cedr_score (document-level log / sums, [CLS] feature, combine layers)."""

    def __init__(self, bert_engine):
        self.be = bert_engine

    def forward(self, doc_input, doc_mask, doc_seg, maxqlen, simmat_layers, mu, sigma, cls_mode, w1, b1, w2=None, b2=None, check=True,
                return_features=False, skip_padding=None):
        """CEDRKNRM_Class.forward (reference CEDRKNRM.py:151-185): int64 [B, P, S] x3 -> fp32 [B].

        skip_padding (default: the encoder engine's setting): as in BertEngine.forward, every passage is encoded at the shortest
        supported length that holds its last attended token.  Padded key positions get an attention weight of exactly 0 and
        padded document columns are masked out of every kernel sum, so the per-passage sums and [CLS] rows are those of the
        full-length computation; only the dead rows and columns are not computed."""
        _need_gpu(doc_input, doc_mask, doc_seg, mu, sigma, w1, b1)
        if cls_mode not in CLS_MODES:
            raise ValueError("cls must be 'avg', 'max' or None")
        ids, mask, seg = _i64(doc_input), _i64(doc_mask), _i64(doc_seg)
        B, P, S = ids.shape
        dev = ids.device
        out = torch.empty(B, dtype=torch.float32, device=dev)
        if B == 0:
            return out
        m = self.be.model()
        lib = _lib.load()
        # in the configured order: the reference concatenates the per-layer features as listed (CEDRKNRM.py:166-168), so the
        # columns of `combine` follow it; -1 alone = no similarity matrices (CEDRKNRM.py:48-52)
        layers = [int(x) for x in simmat_layers if int(x) >= 0]
        n_sel, K, A, H, NP = len(layers), mu.numel(), maxqlen + 1, m.hidden, B * P
        if A + 1 > S:
            raise ValueError("maxqlen + 2 exceeds the passage length")
        # the query mask the reference applies to every passage of a document: its FIRST passage's (CEDRKNRM.py:123)
        qm0 = ((mask[:, 0, 1:A + 1] != 0) & (seg[:, 0, 1:A + 1] == 0)).float().repeat_interleave(P, dim=0).contiguous()   # [NP, A]
        pk = torch.empty((max(1, n_sel), NP, K * A), dtype=torch.float32, device=dev)
        cls = torch.empty((NP, H), dtype=torch.float32, device=dev)
        fids, fmask, fseg = ids.view(NP, S), mask.view(NP, S), seg.view(NP, S)
        if skip_padding is None:
            skip_padding = self.be.skip_padding
        arr = (ctypes.c_int * max(1, n_sel))(*layers)

        def run(bi, bm, bs, Sb, extras_b, outs_b, ws_key):
            (bq,), (pk_b, cls_b), n = extras_b, outs_b, bi.shape[0]
            m, ws, mb = self.be._workspace(ws_key, Sb, n, dev)
            rc = lib.capamd_cedr_passage_features(_ptr(bi), _ptr(bm), _ptr(bs), n, 1, Sb, ctypes.byref(m), mb, _ptr(ws), ws.numel(), int(maxqlen),
                                                  _ptr(bq), arr, n_sel, _ptr(mu), _ptr(sigma), K, _ptr(pk_b), _ptr(cls_b),
                                                  _ptr(status_word(dev).t), _stream())
            _lib.check(rc, "capamd_cedr_passage_features")

        # (a bucket must hold the query columns: Sb > maxqlen + 2)
        self.be._by_length(fids, fmask, fseg, _shorter_lengths(S, skip_padding, A + 1), run, extras=[qm0], outs=[(pk, 1), (cls, 0)])
        n_in = (H if cls_mode else 0) + n_sel * K
        feats = torch.empty((B, n_in), dtype=torch.float32, device=dev) if return_features else None
        hidden = 0 if w2 is None else w1.shape[0]
        rc = lib.capamd_cedr_score(_ptr(pk), _ptr(cls), B, P, int(maxqlen), n_sel, K, H, CLS_MODES[cls_mode], _ptr(w1), _ptr(b1), hidden,
                                   None if w2 is None else _ptr(w2), None if b2 is None else _ptr(b2), _ptr(out),
                                   None if feats is None else _ptr(feats), _stream())
        _lib.check(rc, "capamd_cedr_score")
        if check:
            status_word(dev).raise_if_set()
        return (out, feats) if return_features else out


PARADE_MAX_PASSAGES = 63     # P + 1 rows per document in the aggregation head's attention (csrc/parade.hip)


class ParadeEngine:
    """PARADE (reference ptparade.py, aggregation = "transformer") on top of a BertEngine's packed encoder: capamd_parade_passage_cls
    (encoder; the last layer on the [CLS] rows only; fp32 [CLS] rows of the last hidden state) followed by capamd_parade_head (the two
    BertLayers over [initial_cls; passage rows] + position embeddings, then `linear`, in fp32)."""

    def __init__(self, bert_engine, ln_eps=1e-12):
        self.be = bert_engine
        self.ln_eps = float(ln_eps)
        self._head_ws = None

    def passage_cls(self, ids, mask, seg, skip_padding=None):
        """int64 [B, P, S] x3 -> fp32 [B * P, hidden]: the [CLS] rows of the last hidden state (ptparade.py:74).  skip_padding (default:
        the encoder engine's setting): as in BertEngine.forward, every passage is encoded at the shortest supported length that holds
        its last attended token (the rows are those of the full-length computation), the buckets on side streams; the rows are
        scattered back by index_copy_."""
        B, P, S = ids.shape
        dev, NP = ids.device, B * P
        H = self.be.model().hidden
        cls = torch.empty((NP, H), dtype=torch.float32, device=dev)
        fids, fmask, fseg = ids.view(NP, S), mask.view(NP, S), seg.view(NP, S)
        if skip_padding is None:
            skip_padding = self.be.skip_padding

        def run(bi, bm, bs, Sb, _, outs_b, ws_key):
            n = bi.shape[0]
            m, ws, mb = self.be._workspace(ws_key, Sb, n, dev)
            rc = _lib.load().capamd_parade_passage_cls(_ptr(bi), _ptr(bm), _ptr(bs), n, 1, Sb, ctypes.byref(m), mb, _ptr(ws), ws.numel(),
                                                       _ptr(outs_b[0]), _ptr(status_word(dev).t), _stream())
            _lib.check(rc, "capamd_parade_passage_cls")

        self.be._by_length(fids, fmask, fseg, _shorter_lengths(S, skip_padding), run, outs=[(cls, 0)])
        return cls

    def head(self, cls, B, P, head_params, aggregated=False):
        """capamd_parade_head over fp32 [B * P, hidden] [CLS] rows -> fp32 [B] (and the aggregated rows [B, hidden] if asked).
        head_params: the PTParade_Class state_dict names (``initial_cls_embedding``, ``full_position_embeddings``,
        ``transformer_layer_{1,2}.*``, ``linear.*``) -> live fp32 tensors on the device, read in place."""
        lib = _lib.load()
        keep = {k: _f32(v.detach()) for k, v in head_params.items()}
        _need_gpu(cls, *keep.values())
        H = keep["initial_cls_embedding"].numel()
        if keep["full_position_embeddings"].numel() != (P + 1) * H:
            raise ValueError(f"full_position_embeddings holds {keep['full_position_embeddings'].numel() // H} rows, the documents {P} passages + 1")
        hm = _lib.ParadeHeadModel()
        hm.initial_cls, hm.pos_emb = keep["initial_cls_embedding"].data_ptr(), keep["full_position_embeddings"].data_ptr()
        for i, n in enumerate(_LAYER_TENSORS):
            hm.layer1[i] = keep["transformer_layer_1." + n].data_ptr()
            hm.layer2[i] = keep["transformer_layer_2." + n].data_ptr()
        hm.linear_w, hm.linear_b = keep["linear.weight"].data_ptr(), keep["linear.bias"].data_ptr()
        hm.hidden, hm.heads, hm.ffn, hm.ln_eps = H, H // 64, keep["transformer_layer_1.intermediate.dense.weight"].shape[0], self.ln_eps
        need = lib.capamd_parade_workspace_bytes(ctypes.byref(hm), B, P)
        if need < 0:
            raise ValueError("unsupported PARADE geometry: need hidden == 64*heads <= 1024, ffn % 64 == 0, 1 <= passages <= 63")
        dev = cls.device
        if self._head_ws is None or self._head_ws.numel() < need or self._head_ws.device != dev:
            self._head_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(B, dtype=torch.float32, device=dev)
        agg = torch.empty((B, H), dtype=torch.float32, device=dev) if aggregated else None
        rc = lib.capamd_parade_head(_ptr(cls), B, P, ctypes.byref(hm), _ptr(self._head_ws), self._head_ws.numel(), _ptr(out), _ptr(agg), _stream())
        _lib.check(rc, "capamd_parade_head")
        return (out, agg) if aggregated else out

    def forward(self, doc_input, doc_mask, doc_seg, head_params, return_cls=False, skip_padding=None, check=True):
        """PTParade_Class.forward (reference ptparade.py:66-78): int64 [B, P, S] x3 -> fp32 [B] (and the fp32 [CLS] rows [B * P, hidden]
        with return_cls).  The aggregation layers see every passage, the extractor's padding passages included (no passage mask)."""
        B, P, S = doc_input.shape
        if P < 1 or P > PARADE_MAX_PASSAGES:
            raise ValueError(f"PARADE scores 1 to {PARADE_MAX_PASSAGES} passages per document (P + 1 <= 64 rows in the aggregation head); got {P}")
        _need_gpu(doc_input, doc_mask, doc_seg)
        ids, mask, seg = _i64(doc_input), _i64(doc_mask), _i64(doc_seg)
        dev = ids.device
        if B == 0:
            out = torch.empty(0, dtype=torch.float32, device=dev)
            return (out, torch.empty((0, self.be.model().hidden), device=dev)) if return_cls else out
        cls = self.passage_cls(ids, mask, seg, skip_padding)
        out = self.head(cls, B, P, head_params)
        if check:
            status_word(dev).raise_if_set()
        return (out, cls) if return_cls else out


BIRCH_MAX_PASSAGES = 64      # a document's passages are the lanes of one wave (csrc/birch.hip)
BIRCH_MAX_HIDDEN = 256
BIRCH_TRUNCATE = {"none": 0, "reference": 1}


class BirchEngine:
    """Birch (reference birch.py:72-127) on top of a BertEngine whose pooler / classifier are BertForNextSentencePrediction's:
    capamd_birch_plan (which passages are encoded, compacted, their masks cleared behind the sub-batch's cut) -> the passage encoder
    over the compacted rows -> capamd_birch_head (fill, top-k, combine).

    truncate = "reference": a passage is scored up to the cut the reference slices its sub-batch at (:106-109) - with the torch of
    today the first token of segment B, so `[CLS] q [SEP] t1` is all the encoder sees; the cut depends on `subbatch`, the reference's
    batch size.  truncate = "none": the whole passage, as the commented-out loop (:110-115) would have it."""

    def __init__(self, bert_engine, truncate="reference"):
        if truncate not in BIRCH_TRUNCATE:
            raise ValueError(f"truncate must be one of {sorted(BIRCH_TRUNCATE)}; got {truncate!r}")
        self.be = bert_engine
        self.truncate = truncate
        self._plan_ws = None

    @staticmethod
    def check_dims(P, S, topk, hidden, subbatch=1):
        """the refusals of capamd_birch_plan / capamd_birch_head, by name, before any device work"""
        if not 1 <= P <= BIRCH_MAX_PASSAGES:
            raise ValueError(f"Birch scores 1 to {BIRCH_MAX_PASSAGES} passages per document (numpassages); got {P}")
        if not 1 <= topk <= P:
            raise ValueError(f"topk must lie in 1..numpassages = {P} (torch.topk over a document's passage scores, birch.py:81); got topk = {topk}")
        if not 0 <= hidden <= BIRCH_MAX_HIDDEN:
            raise ValueError(f"hidden must lie in 0..{BIRCH_MAX_HIDDEN}; got {hidden}")
        if subbatch < 1:
            raise ValueError(f"subbatch must be at least 1; got {subbatch}")
        if S not in SUPPORTED_LENGTHS:
            raise ValueError(f"unsupported passage length {S} (supported: multiples of 32 up to 256, 384, 512)")

    def plan(self, ids, mask, seg, subbatch, truncate=None):
        """int64 [B, P, S] x3 -> (enc_ids, enc_mask, enc_seg int64 [n_enc, S], doc_first int32 [B + 1]).  Reads n_enc back: the one host
        round trip of a call before the encoder's own (the bucket sizes)."""
        truncate = self.truncate if truncate is None else truncate
        if truncate not in BIRCH_TRUNCATE:
            raise ValueError(f"truncate must be one of {sorted(BIRCH_TRUNCATE)}; got {truncate!r}")
        B, P, S = ids.shape
        self.check_dims(P, S, 1, 0, subbatch)
        _need_gpu(ids, mask, seg)
        ids, mask, seg = _i64(ids), _i64(mask), _i64(seg)
        dev = ids.device
        if B == 0:
            none = torch.empty((0, S), dtype=torch.int64, device=dev)
            return none, none, none, torch.zeros(1, dtype=torch.int32, device=dev)
        lib = _lib.load()
        need = lib.capamd_birch_workspace_bytes(B, P)
        if need < 0:
            raise ValueError(f"Birch: {B} documents of {P} passages are more than one call takes (B P < 2^31)")
        if self._plan_ws is None or self._plan_ws.numel() < need or self._plan_ws.device != dev:
            self._plan_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        enc = [torch.empty((B * P, S), dtype=torch.int64, device=dev) for _ in range(3)]
        doc_first = torch.empty(B + 1, dtype=torch.int32, device=dev)
        n_enc = torch.empty(1, dtype=torch.int32, device=dev)
        rc = lib.capamd_birch_plan(_ptr(ids), _ptr(mask), _ptr(seg), B, P, S, int(subbatch), BIRCH_TRUNCATE[truncate], _ptr(self._plan_ws),
                                   self._plan_ws.numel(), _ptr(enc[0]), _ptr(enc[1]), _ptr(enc[2]), _ptr(doc_first), _ptr(n_enc), _stream())
        _lib.check(rc, "capamd_birch_plan")
        n = int(n_enc.item())
        return enc[0][:n], enc[1][:n], enc[2][:n], doc_first

    def passage_logits(self, enc_ids, enc_mask, enc_seg, skip_padding=None, check=True):
        """the compacted rows int64 [n, S] x3 -> fp32 [n]: logit 1 of the next-sentence head, by the MaxP encoder path (P = 1, "first")"""
        n, S = enc_ids.shape
        if n == 0:
            return torch.empty(0, dtype=torch.float32, device=enc_ids.device)
        shape = (n, 1, S)
        return self.be.forward(enc_ids.view(shape), enc_mask.view(shape), enc_seg.view(shape), "first", return_passage_logits=True, check=check,
                               skip_padding=skip_padding)[1]

    @staticmethod
    def head(logits, doc_first, B, P, topk, combine, details=False):
        """capamd_birch_head: fp32 [n] logits of the compacted rows + doc_first -> fp32 [B] (details: also the top-k values [B, topk] and
        the passage scores [B, P] in the reference's layout).  combine: the state_dict names of Birch_Class.combine (``combine.weight``, or
        ``combine.0.*`` and ``combine.2.*``) -> live fp32 tensors on the device, read in place."""
        keep = {k: _f32(v.detach()) for k, v in combine.items()}
        logits = _f32(logits)
        _need_gpu(logits, doc_first, *keep.values())
        if "combine.weight" in keep:
            hidden, w1, b1, w2, b2 = 0, keep["combine.weight"], None, None, None
        else:
            w1, b1, w2, b2 = (keep[k] for k in ("combine.0.weight", "combine.0.bias", "combine.2.weight", "combine.2.bias"))
            hidden = w1.shape[0]
        BirchEngine.check_dims(P, SUPPORTED_LENGTHS[0], topk, hidden)
        if w1.numel() != max(hidden, 1) * topk:
            raise ValueError(f"combine takes {w1.numel() // max(hidden, 1)} features, topk is {topk}")
        dev = logits.device
        out = torch.empty(B, dtype=torch.float32, device=dev)
        top = torch.empty((B, topk), dtype=torch.float32, device=dev) if details else None
        scores = torch.empty((B, P), dtype=torch.float32, device=dev) if details else None
        if B == 0:
            return (out, top, scores) if details else out
        rc = _lib.load().capamd_birch_head(_ptr(logits), logits.numel(), _ptr(_i32(doc_first)), B, P, topk, hidden, _ptr(w1), _ptr(b1), _ptr(w2),
                                           _ptr(b2), _ptr(out), _ptr(top), _ptr(scores), _stream())
        _lib.check(rc, "capamd_birch_head")
        return (out, top, scores) if details else out

    def forward(self, doc, mask, seg, topk, combine, subbatch=None, truncate=None, details=False, skip_padding=None, check=True):
        """Birch_Class.forward (birch.py:72-83): int64 [B, P, S] x3 -> fp32 [B]; details: (out, top-k values [B, topk], passage scores
        [B, P], the compacted rows' logits [n_enc], doc_first).  subbatch (default: B, what the reference uses): passages per
        sub-batch under truncate = "reference"."""
        B, P, S = doc.shape
        hidden = 0 if "combine.weight" in combine else combine["combine.0.weight"].shape[0]
        subbatch = max(B, 1) if subbatch is None else int(subbatch)
        self.check_dims(P, S, topk, hidden, subbatch)
        _need_gpu(doc, mask, seg)
        enc_ids, enc_mask, enc_seg, doc_first = self.plan(doc, mask, seg, subbatch, truncate)
        logits = self.passage_logits(enc_ids, enc_mask, enc_seg, skip_padding, check)
        res = self.head(logits, doc_first, B, P, topk, combine, details)
        return (*res, logits, doc_first) if details else res


class _PerDocumentEngine:
    """What the engines of the per-document rerankers share: the documents of a call run in micro-batches of `docs_per_microbatch`
    (None: as many as the model's budget holds) on one workspace that only ever grows."""

    def __init__(self, docs_per_microbatch=None):
        self.docs_per_microbatch = docs_per_microbatch
        self._ws = None

    @staticmethod
    def _ids(query, doc):
        _need_gpu(query, doc)
        q, d = _i64(query), _i64(doc)
        B, Q = q.shape
        if d.shape[0] != B:
            raise ValueError(f"{B} query rows for {d.shape[0]} documents")
        return q, d, B, Q, d.shape[1]

    @staticmethod
    def _fit(bytes_of, B, budget):
        """the default micro-batch: as many documents as the budget holds, by what the second document adds to the first"""
        return max(1, budget // max(1, bytes_of(2) - bytes_of(1)))

    def _workspace(self, bytes_fn, m, device, B, Q, L, budget, refusal):
        """-> (documents per micro-batch, the workspace that holds them) by the model's capamd_*_workspace_bytes; ValueError(refusal())
        for a geometry the entry does not take"""
        def bytes_of(nb):
            return bytes_fn(ctypes.byref(m), nb, Q, L)

        if bytes_of(1) < 0:
            raise ValueError(refusal())
        nb = self.docs_per_microbatch
        if nb is None:
            nb = self._fit(bytes_of, B, budget)
        nb = max(1, min(int(nb), max(B, 1)))
        need = bytes_of(nb)
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        return nb, self._ws

    @staticmethod
    def _finish(rc, what, st, check):
        _lib.check(rc, what)
        if check:
            st.raise_if_set()


TK_WORKSPACE_BUDGET = 1 << 30      # bytes of activations per capamd_tk_forward call (documents run in micro-batches that fit)


def _up64(n):
    return (n + 63) // 64 * 64


class TKEngine(_PerDocumentEngine):
    """TK (reference TK.py, TK_class.forward) through capamd_tk_forward.  The encoder's weights are re-laid out once per set of weights
    into the padded layout of include/capreolus_amd.h (each head in its own 16-multiple slot, widths padded to 64 with zeros), kept
    until any parameter changes (storage pointers + version counters, as ConvProjectionTables); the embedding table and the `pe`
    buffer are read in place.  `docs_per_microbatch` (None: as many as TK_WORKSPACE_BUDGET holds) bounds the activations of a call."""

    def __init__(self, docs_per_microbatch=None):
        super().__init__(docs_per_microbatch)
        self._key = None
        self._keep = None

    @staticmethod
    def _layer_names(n):
        pre = f"transformer_encoder.layers.{n}."
        return [pre + s for s in ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
                                  "norm1.weight", "norm1.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                                  "norm2.weight", "norm2.bias")]

    def _pack(self, params, heads, numlayers):
        """the padded per-layer tensors (a list of 12 per layer, in capamd_tk_layer's order) and the TkLayer host array"""
        D = params["embedding.weight"].shape[1]
        F = params[self._layer_names(0)[6]].shape[0]
        hd = D // heads
        hs = (hd + 15) // 16 * 16
        Dp, Fp, Hs = _up64(D), _up64(F), _up64(heads * hs)
        dev = params["embedding.weight"].device
        j = torch.arange(hd, device=dev)
        h = torch.arange(heads, device=dev)
        dst_h = (h[:, None] * hs + j[None, :]).reshape(-1)          # head slot columns / rows
        src_h = (h[:, None] * hd + j[None, :]).reshape(-1)
        dst_qkv = torch.cat([p * Hs + dst_h for p in range(3)])
        src_qkv = torch.cat([p * D + src_h for p in range(3)])

        def vec(t, n):
            out = torch.zeros(n, dtype=torch.float32, device=dev)
            out[: t.numel()] = t.reshape(-1)
            return out

        def mat(t, rows, cols):
            out = torch.zeros(rows, cols, dtype=torch.float32, device=dev)
            out[: t.shape[0], : t.shape[1]] = t
            return out

        tensors, layers = [], (_lib.TkLayer * numlayers)()
        for n in range(numlayers):
            in_w, in_b, out_w, out_b, g1, b1n, w1, b1, w2, b2, g2, b2n = (_f32(params[k].detach()) for k in self._layer_names(n))
            wqkv = torch.zeros(3 * Hs, Dp, dtype=torch.float32, device=dev)
            wqkv[dst_qkv, :D] = in_w[src_qkv]
            bqkv = torch.zeros(3 * Hs, dtype=torch.float32, device=dev)
            bqkv[dst_qkv] = in_b[src_qkv]
            wo = torch.zeros(Dp, Hs, dtype=torch.float32, device=dev)
            wo[:D, dst_h] = out_w[:, src_h]
            ts = [wqkv, bqkv, wo, vec(out_b, Dp), vec(g1, Dp), vec(b1n, Dp), mat(w1, Fp, Dp), vec(b1, Fp), mat(w2, Dp, Fp), vec(b2, Dp),
                  vec(g2, Dp), vec(b2n, Dp)]
            ts = [t.contiguous() for t in ts]
            for name, t in zip(_lib.TkLayer._fields_, ts):
                setattr(layers[n], name[0], t.data_ptr())
            tensors += ts
        return tensors, layers

    def model(self, params, heads, numlayers, usemask, alpha, pad, ln_eps, mixer=None):
        """the capamd_tk_model of these live parameters (packing the encoder again only when a parameter changed)"""
        names = [k for n in range(numlayers) for k in self._layer_names(n)]
        _need_gpu(*(params[k] for k in names))
        key = tuple((params[k].data_ptr(), params[k]._version) for k in names) + (heads, numlayers)
        if key != self._key:
            self._keep = self._pack(params, heads, numlayers)
            self._key = key
        tensors, layers = self._keep
        emb, pe = _f32(params["embedding.weight"].detach()), _f32(params["position_encoder.pe"].detach())
        heads_w = [_f32(params[k].detach()).reshape(-1) for k in ("s_log_fcc.weight", "s_len_fcc.weight", "comb_fcc.weight")]
        mix = None if mixer is None else _f32(mixer.detach()).reshape(-1)
        _need_gpu(emb, pe, *heads_w)
        m = _lib.TkModel()
        m.emb, m.pe, m.layers_host = emb.data_ptr(), pe.data_ptr(), ctypes.cast(layers, ctypes.c_void_p)
        m.mixer = None if mix is None else mix.data_ptr()
        m.s_log_w, m.s_len_w, m.comb_w = (t.data_ptr() for t in heads_w)
        m.vocab, m.pad = emb.shape[0], int(pad)
        m.dim, m.heads, m.ffdim, m.numlayers = emb.shape[1], int(heads), params[self._layer_names(0)[6]].shape[0], int(numlayers)
        m.max_len, m.usemask, m.alpha, m.ln_eps = pe.shape[0], int(bool(usemask)), float(alpha), float(ln_eps)
        return m, (emb, pe, heads_w, mix, layers, tensors)     # (the second item keeps what m points to alive)

    def forward(self, query, doc, params, heads, numlayers, usemask, alpha, pad, ln_eps=1e-5, mixer=None, features=False, check=True):
        """int64 query ids [B, Q], document ids [B, L] -> fp32 scores [B] (and the [B, 22] features s_log_k | s_len_k with features=True)"""
        q, d, B, Q, L = self._ids(query, doc)
        m, keep = self.model(params, heads, numlayers, usemask, alpha, pad, ln_eps, mixer)
        lib = _lib.load()
        nb, ws = self._workspace(lib.capamd_tk_workspace_bytes, m, q.device, B, Q, L, TK_WORKSPACE_BUDGET, lambda: (
                                 f"unsupported TK geometry: dim {m.dim}, heads {m.heads}, ffdim {m.ffdim}, layers {m.numlayers}, Q {Q}, L {L} "
                                 f"(dim <= 512, dim % heads == 0, dim / heads <= 64, ffdim <= 512, layers >= 1, Q <= 32, L <= {m.max_len})"))
        out = torch.empty(B, dtype=torch.float32, device=q.device)
        feats = torch.empty((B, 22), dtype=torch.float32, device=q.device) if features else None
        st = status_word(q.device)
        rc = lib.capamd_tk_forward(_ptr(q), _ptr(d), B, Q, L, ctypes.byref(m), nb, _ptr(ws), ws.numel(), _ptr(out), _ptr(feats), _ptr(st.t), _stream())
        self._finish(rc, "capamd_tk_forward", st, check)
        return (out, feats) if features else out


HINT_WORKSPACE_BUDGET = 1 << 30    # bytes of window-transposed inputs per capamd_hint_forward call (documents run in micro-batches that fit)


class HintEngine(_PerDocumentEngine):
    """HINT (reference HINT.py, HiNT_main.test_forward) through capamd_hint_forward.  Every parameter is read in place from the live
    tensors (nn.Linear / nn.LSTM layout): there is nothing to re-lay out and so nothing cached but the workspace.
    `docs_per_microbatch` (None: as many as HINT_WORKSPACE_BUDGET holds) bounds the workspace of a call."""

    _FIELDS = (("emb", "HiNT1.embedding.weight"), ("ws_w", "HiNT1.Ws.weight"), ("ws_b", "HiNT1.Ws.bias")) + tuple(
        (f"{g}_{f}_{k[0]}", f"HiNT1.{mod}.gru_cell.{lin}.{k}") for g, mod in (("gru1", "GRU2d1"), ("gru3", "GRU2d3"))
        for f, lin in (("wrz", "Wrz"), ("w", "W"), ("u", "U")) for k in ("weight", "bias")) + tuple(
        (f"lstm_{k[0]}_{k[1]}{'_r' if rev else ''}", f"HiNT1.lstm.{'weight' if k[0] == 'w' else 'bias'}_{k[1]}_l0{rev}")
        for rev in ("", "_reverse") for k in (("w", "ih"), ("w", "hh"), ("b", "ih"), ("b", "hh"))) + (
        ("wv_w", "HiNT1.Wv.weight"), ("wv_b", "HiNT1.Wv.bias"), ("fc_w", "HiNT1.fc.weight"), ("fc_b", "HiNT1.fc.bias"))

    def model(self, params, kmax):
        """the capamd_hint_model of these live parameters (the second item keeps what it points to alive)"""
        keep = {f: _f32(params[name].detach()) for f, name in self._FIELDS}
        _need_gpu(*keep.values())
        m = _lib.HintModel()
        for f, t in keep.items():
            setattr(m, f, t.data_ptr())
        m.vocab, m.dim, m.kmax = keep["emb"].shape[0], keep["emb"].shape[1], int(kmax)
        return m, keep

    def forward(self, query, doc, params, kmax, evidence=False, check=True):
        """int64 query ids [B, Q], document ids [B, L] -> fp32 scores [B] (and the [B, L // 100, 8] window evidence with evidence=True)"""
        q, d, B, Q, L = self._ids(query, doc)
        m, keep = self.model(params, kmax)
        lib = _lib.load()
        nb, ws = self._workspace(lib.capamd_hint_workspace_bytes, m, q.device, B, Q, L, HINT_WORKSPACE_BUDGET, lambda: (
                                 f"unsupported HINT geometry: dim {m.dim}, kmax {m.kmax}, Q {Q}, L {L} "
                                 f"(dim <= 512, Q <= 32, 100 <= L, L // 100 <= 64, 1 <= kmax <= min(2 (L // 100), 32))"))
        out = torch.empty(B, dtype=torch.float32, device=q.device)
        ev = torch.empty((B, L // 100, 8), dtype=torch.float32, device=q.device) if evidence else None
        st = status_word(q.device)
        rc = lib.capamd_hint_forward(_ptr(q), _ptr(d), B, Q, L, ctypes.byref(m), nb, _ptr(ws), ws.numel(), _ptr(out), _ptr(ev), _ptr(st.t), _stream())
        self._finish(rc, "capamd_hint_forward", st, check)
        return (out, ev) if evidence else out


POSIT_WORKSPACE_BUDGET = 6 << 30    # bytes of activations per capamd_posit_forward call: 1000 pairs of 4 x 800 terms at dim 300 fit at once


class PositEngine(_PerDocumentEngine):
    """POSITDRMM (reference POSITDRMM.py, POSITDRMM_class.test_forward) through capamd_posit_forward.  The LSTM's weights are packed
    into the kernels' padded, gate-interleaved layout once per parameter version (include/capreolus_amd.h); the embedding table, Q1 and
    Wg are read in place.  `docs_per_microbatch` (None: B in as few equal parts as POSIT_WORKSPACE_BUDGET allows) bounds the workspace."""

    _LSTM = tuple(f"posit1.encoding_layer.{k}_l{n}{rev}" for n in (0, 1) for rev in ("", "_reverse")
                  for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))

    def __init__(self, docs_per_microbatch=None):
        super().__init__(docs_per_microbatch)
        self._key = None
        self._keep = None

    @staticmethod
    def _fit(bytes_of, B, budget):
        """B in as few equal parts as the budget allows, beside the 512 MiB projection chunk; what a pair adds is read between large
        micro-batches, where that chunk has reached its fixed size"""
        per_doc = max(1, (bytes_of(1 << 16) - bytes_of(1 << 15)) >> 15)
        most = max(1, (budget - (512 << 20)) // per_doc)
        parts = -(-max(B, 1) // most)
        return -(-max(B, 1) // parts)

    @staticmethod
    def _pack(params, D):
        """per layer (w_ih [2, 4 Dp, K], w_hh [2, 4 Dp, Dp], bias [2, 4 Dp]), zero-padded, gate rows reordered"""
        Dp = (D + 63) // 64 * 64
        dev = params[PositEngine._LSTM[0]].device
        p = torch.arange(4 * Dp, device=dev)
        unit, gate = (p // 64) * 16 + p % 16, (p % 64) // 16
        dst = p[unit < D]
        src = (gate * D + unit)[unit < D]
        out = []
        for n in (0, 1):
            K = Dp * (n + 1)
            w_ih = torch.zeros(2, 4 * Dp, K, dtype=torch.float32, device=dev)
            w_hh = torch.zeros(2, 4 * Dp, Dp, dtype=torch.float32, device=dev)
            bias = torch.zeros(2, 4 * Dp, dtype=torch.float32, device=dev)
            for d, rev in enumerate(("", "_reverse")):
                wi, wh, bi, bh = (_f32(params[f"posit1.encoding_layer.{k}_l{n}{rev}"].detach())
                                  for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                for half in range(n + 1):                      # layer 1 reads [forward half, backward half], each in its own Dp columns
                    w_ih[d, dst, half * Dp: half * Dp + D] = wi[src, half * D: (half + 1) * D]
                w_hh[d, dst, :D] = wh[src]
                bias[d, dst] = bi[src] + bh[src]
            # W_hh fragment-major, [direction][unit block][k / 16][gate][lane = 16 (k % 16 // 4) + unit % 16][4]: a wave's load is contiguous
            w_hh = w_hh.view(2, Dp // 16, 4, 16, Dp // 16, 4, 4).permute(0, 1, 4, 2, 5, 3, 6).contiguous()
            out.append((w_ih, w_hh, bias))
        return out

    def model(self, params, pad):
        """the capamd_posit_model of these live parameters (packing the LSTM again only when one of its parameters changed)"""
        emb = _f32(params["posit1.embedding.weight"].detach())
        heads = [_f32(params[k].detach()).reshape(-1) for k in ("posit1.Q1.weight", "posit1.Q1.bias", "posit1.Wg.weight", "posit1.Wg.bias")]
        _need_gpu(emb, *heads, *(params[k] for k in self._LSTM))
        key = tuple((params[k].data_ptr(), params[k]._version) for k in self._LSTM)
        if key != self._key:
            self._keep = self._pack(params, emb.shape[1])
            self._key = key
        m = _lib.PositModel()
        m.emb = emb.data_ptr()
        for n, (w_ih, w_hh, bias) in enumerate(self._keep):
            m.w_ih[n], m.w_hh[n], m.bias[n] = w_ih.data_ptr(), w_hh.data_ptr(), bias.data_ptr()
        m.q1_w, m.q1_b, m.wg_w, m.wg_b = (t.data_ptr() for t in heads)
        m.vocab, m.pad, m.dim = emb.shape[0], int(pad), emb.shape[1]
        return m, (emb, heads, self._keep)     # (the second item keeps what m points to alive)

    def forward(self, query, query_idf, doc, params, pad, extras=None, bm25=None, details=False, check=True):
        """int64 query ids [B, Q], fp32 idf [B, Q], document ids [B, L]; extras [B, 4], or bm25 [B] (the three match statistics are then
        the kernel's own) -> fp32 scores [B]; with details=True also a dict of features [B, Q, 6], stats [B, 3], query_context
        [B, Q, 2 dim] and doc_context [B, L, 2 dim]"""
        _need_gpu(query, query_idf, doc, extras, bm25)
        if (extras is None) == (bm25 is None):
            raise ValueError("give either extras [B, 4] or bm25 [B]")
        q, d, idf = _i64(query), _i64(doc), _f32(query_idf)
        B, Q = q.shape
        L = d.shape[1]
        side = _f32(extras).reshape(-1) if extras is not None else _f32(bm25).reshape(-1)
        if d.shape[0] != B or tuple(idf.shape) != (B, Q) or side.numel() != (4 * B if extras is not None else B):
            raise ValueError(f"{B} query rows of {Q} terms for {d.shape[0]} documents, idf {tuple(idf.shape)}, {side.numel()} extra values")
        m, keep = self.model(params, pad)
        lib = _lib.load()
        nb, ws = self._workspace(lib.capamd_posit_workspace_bytes, m, q.device, B, Q, L, POSIT_WORKSPACE_BUDGET, lambda: (
            f"unsupported POSITDRMM geometry: dim {m.dim}, Q {Q}, L {L} (dim <= 320, Q <= 16, 5 <= L <= 8192)"))
        out = torch.empty(B, dtype=torch.float32, device=q.device)
        det = None
        if details:
            D = m.dim
            det = {"features": torch.empty((B, Q, 6), dtype=torch.float32, device=q.device),
                   "stats": torch.empty((B, 3), dtype=torch.float32, device=q.device),
                   "query_context": torch.empty((B, Q, 2 * D), dtype=torch.float32, device=q.device),
                   "doc_context": torch.empty((B, L, 2 * D), dtype=torch.float32, device=q.device)}
        st = status_word(q.device)
        rc = lib.capamd_posit_forward(_ptr(q), _ptr(idf), _ptr(d), _ptr(side) if extras is not None else None, _ptr(side) if extras is None else None,
                                      B, Q, L, ctypes.byref(m), nb, _ptr(ws), ws.numel(), _ptr(out),
                                      *((_ptr(det[k]) for k in ("features", "stats", "query_context", "doc_context")) if details else (None,) * 4),
                                      _ptr(st.t), _stream())
        self._finish(rc, "capamd_posit_forward", st, check)
        return (out, det) if details else out


class DeepTileEngine(_PerDocumentEngine):
    """DeepTileBar (reference DeepTileBar.py, DeepTileBar_class.test_forward; deeptileextractor.py, color_grid) through
    capamd_deeptile_forward and capamd_deeptile_color.  The ten convolutions, ten LSTMs and three linear layers are laid out into the one
    buffer of include/capreolus_amd.h once per set of weights, kept until any parameter changes (storage pointers + version counters, as
    TKEngine); the embedding table of the colouring is read in place.  Neither call needs a workspace."""

    WIDTHS = tuple(range(1, 11))

    def __init__(self):
        super().__init__()
        self._key = None
        self._keep = None

    @classmethod
    def names(cls):
        """the state_dict names in the packed order"""
        pre = "DeepTileBar1."
        out = []
        for w in cls.WIDTHS:
            out += [f"{pre}conv{w}.weight", f"{pre}conv{w}.bias"] + [f"{pre}lstm{w}.{k}_l0" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return out + [f"{pre}W{n}.{k}" for n in (1, 2, 3) for k in ("weight", "bias")]

    def model(self, params):
        """the capamd_deeptile_model of these live parameters (packing again only when a parameter changed); the second item keeps what
        it points to alive"""
        names = self.names()
        _need_gpu(*(params[k] for k in names))
        key = tuple((params[k].data_ptr(), params[k]._version) for k in names)
        if key != self._key:
            self._keep = torch.cat([_f32(params[k].detach()).reshape(-1) for k in names])
            self._key = key
        conv, w_hh, w1, w2 = (params[f"DeepTileBar1.{k}"] for k in ("conv1.weight", "lstm1.weight_hh_l0", "W1.weight", "W2.weight"))
        m = _lib.DeepTileModel()
        m.packed, m.packed_floats = self._keep.data_ptr(), self._keep.numel()
        m.filters, m.channels, m.maxqlen = conv.shape[0], conv.shape[1], conv.shape[2]
        m.hidden, m.lin1, m.lin2 = w_hh.shape[1], w1.shape[0], w2.shape[0]
        return m, self._keep

    def forward(self, tiles, params, evidence=False):
        """fp32 tiles [B, Q, P, C] -> fp32 scores [B] (and the [B, 10, hidden] last hidden states, the input of W1, with evidence=True)"""
        _need_gpu(tiles)
        if tiles.dim() != 4:
            raise ValueError(f"tiles are [B, Q, P, C]; got {tuple(tiles.shape)}")
        t = _f32(tiles)
        B, Q, P, C = t.shape
        m, keep = self.model(params)
        lib = _lib.load()
        if lib.capamd_deeptile_packed_floats(ctypes.byref(m)) != m.packed_floats or Q != m.maxqlen or C != m.channels or not 10 <= P <= 64:
            raise ValueError(f"unsupported DeepTileBar geometry: tiles Q {Q}, P {P}, C {C} for a model of maxqlen {m.maxqlen}, {m.channels} channels, "
                             f"{m.filters} filters, hidden {m.hidden}, linear {m.lin1} / {m.lin2} (Q and C as the model's, 10 <= P <= 64, "
                             f"maxqlen <= 32, C in (2, 3), 3 filters, hidden <= 16, linear widths <= 128)")
        out = torch.empty(B, dtype=torch.float32, device=t.device)
        ev = torch.empty((B, 10, m.hidden), dtype=torch.float32, device=t.device) if evidence else None
        rc = lib.capamd_deeptile_forward(_ptr(t), B, Q, P, C, ctypes.byref(m), _ptr(out), _ptr(ev), _stream())
        _lib.check(rc, "capamd_deeptile_forward")
        return (out, ev) if evidence else out

    def color(self, query, doc, seg_start, idf, emb, channels=3, check=True):
        """int64 query ids [B, Q], document ids [B, L], int32 segment offsets [B, P + 1], fp32 idf [B, Q], the fp32 table [V, D] -> fp32
        tiles [B, Q, P, channels].  With check=True an id >= V raises IdRangeError and a clamped offset ValueError; with check=False the
        tiles come back and the bits stay in the device's status word."""
        _need_gpu(seg_start, idf, emb)
        q, d, B, Q, L = self._ids(query, doc)
        seg, w, e = _i32(seg_start), _f32(idf), _f32(emb)
        P = seg.shape[1] - 1
        if seg.shape[0] != B or tuple(w.shape) != (B, Q) or e.dim() != 2:
            raise ValueError(f"{B} documents with segment offsets {tuple(seg.shape)}, idf {tuple(w.shape)}, table {tuple(e.shape)}")
        if not (1 <= Q <= 32 and 1 <= P <= 64 and 1 <= e.shape[1] <= 512 and L >= 1 and channels in (2, 3)):
            raise ValueError(f"unsupported colouring geometry: Q {Q}, P {P}, dim {e.shape[1]}, L {L}, channels {channels} "
                             f"(Q <= 32, P <= 64, dim <= 512, channels in (2, 3))")
        tiles = torch.empty((B, Q, P, channels), dtype=torch.float32, device=q.device)
        st = status_word(q.device)
        rc = _lib.load().capamd_deeptile_color(_ptr(q), _ptr(d), _ptr(seg), _ptr(w), B, Q, L, P, _ptr(e), e.shape[0], e.shape[1], channels, _ptr(tiles),
                                               _ptr(st.t), _stream())
        self._finish(rc, "capamd_deeptile_color", st, check)
        return tiles


DUET_WORKSPACE_BUDGET = 1 << 30    # bytes of per-token projections per capamd_duet_forward call (documents run in micro-batches that fit)


class DuetEngine(_PerDocumentEngine):
    """DUET (reference DUET.py, DUET_class.forward) through capamd_duet_forward.  Two weights are re-laid out once per parameter version
    (storage pointers + version counters, as DeepTileEngine): the local model's convolution transposed to [maxdoclen, H], and d_conv1 as
    per-token projections [dim up to 32, 3 H up to 16] (include/capreolus_amd.h); everything else is read in place.
    `activation` ("relu" / "tanh") and `idfweight` are the plugin's config; `docs_per_microbatch` (None: as many as DUET_WORKSPACE_BUDGET
    holds) bounds the workspace of a call."""

    _FIELDS = (("emb", "dm.embedding.weight"), ("lm_b", "lm.conv.0.bias"), ("lm_w0", "lm.ffw.0.weight"), ("lm_b0", "lm.ffw.0.bias"),
               ("lm_w3", "lm.ffw.3.weight"), ("lm_b3", "lm.ffw.3.bias"), ("q_w", "dm.q_conv.0.weight"), ("q_b", "dm.q_conv.0.bias"),
               ("qf_w", "dm.q_ffw.0.weight"), ("qf_b", "dm.q_ffw.0.bias"), ("d_b1", "dm.d_conv1.0.bias"), ("d_w2", "dm.d_conv2.0.weight"),
               ("d_b2", "dm.d_conv2.0.bias"), ("f1_w", "dm.ffw_1.0.weight"), ("f1_b", "dm.ffw_1.0.bias"), ("f2_w", "dm.ffw_2.1.weight"),
               ("f2_b", "dm.ffw_2.1.bias"))
    _PACKED = ("lm.conv.0.weight", "dm.d_conv1.0.weight")

    def __init__(self, activation="relu", idfweight=True, docs_per_microbatch=None):
        super().__init__(docs_per_microbatch)
        self.activation = {"relu": 0, "tanh": 1}[activation]
        self.idfweight = int(bool(idfweight))
        self._key = None
        self._packed = None

    @staticmethod
    def _pack(lm_w, d_w1):
        """(lm.conv.0.weight [H, 1, 1, L] -> [L, H]; dm.d_conv1.0.weight [H, 1, 3, dim] -> [dim up to 32, 3 H up to 16], column j H + h)"""
        H, _, _, D = d_w1.shape
        w1t = torch.zeros((D + 31) // 32 * 32, (3 * H + 15) // 16 * 16, dtype=torch.float32, device=d_w1.device)
        w1t[:D, :3 * H] = _f32(d_w1.detach()).view(H, 3, D).permute(2, 1, 0).reshape(D, 3 * H)
        return _f32(lm_w.detach()).view(lm_w.shape[0], -1).t().contiguous(), w1t

    def model(self, params):
        """the capamd_duet_model of these live parameters (re-laying out the two packed weights only when one of them changed); the second
        item keeps what it points to alive"""
        keep = {f: _f32(params[name].detach()) for f, name in self._FIELDS}
        _need_gpu(*keep.values(), *(params[k] for k in self._PACKED))
        key = tuple((params[k].data_ptr(), params[k]._version) for k in self._PACKED)
        if key != self._key:
            self._packed = self._pack(*(params[k] for k in self._PACKED))
            self._key = key
        m = _lib.DuetModel()
        for f, t in keep.items():
            setattr(m, f, t.data_ptr())
        m.lm_wt, m.d_w1t = (t.data_ptr() for t in self._packed)
        m.vocab, m.dim = keep["emb"].shape
        m.nfilters, m.lmhidden = keep["d_b1"].shape[0], keep["lm_b0"].shape[0]
        m.maxdoclen, m.nhidden = self._packed[0].shape[0], keep["f1_w"].shape[1]
        m.activation, m.idfweight = self.activation, self.idfweight
        return m, (keep, self._packed)

    def forward(self, query, query_idf, doc, params, parts=False, evidence=False, check=True):
        """int64 query ids [B, 4], fp32 idf [B, 4], document ids [B, L] -> fp32 scores [B]; with parts=True also (lm, dm) [B, 2]; with
        evidence=True also the query vector [B, H] and the pooled map [B, H, L - 101] (views of one buffer)"""
        _need_gpu(query_idf)
        q, d, B, Q, L = self._ids(query, doc)
        idf = _f32(query_idf)
        if tuple(idf.shape) != (B, Q):
            raise ValueError(f"{B} query rows of {Q} terms with idf {tuple(idf.shape)}")
        m, keep = self.model(params)
        lib = _lib.load()
        nb, ws = self._workspace(lib.capamd_duet_workspace_bytes, m, q.device, B, Q, L, DUET_WORKSPACE_BUDGET, lambda: (
            f"unsupported DUET geometry: Q {Q}, L {L}, nfilters {m.nfilters}, lmhidden {m.lmhidden}, dim {m.dim}, maxdoclen {m.maxdoclen}, "
            f"nhidden {m.nhidden} (Q == 4, 2 <= nfilters <= 32, 1 <= lmhidden <= 256, dim <= 512, 103 <= L <= 8192, L == maxdoclen, "
            f"nhidden == L - 101)"))
        H, NP = m.nfilters, L - 101
        out = torch.empty(B, dtype=torch.float32, device=q.device)
        pt = torch.empty((B, 2), dtype=torch.float32, device=q.device) if parts else None
        ev = torch.empty((B, H, NP + 1), dtype=torch.float32, device=q.device) if evidence else None
        st = status_word(q.device)
        rc = lib.capamd_duet_forward(_ptr(q), _ptr(d), _ptr(idf), B, Q, L, ctypes.byref(m), nb, _ptr(ws), ws.numel(), _ptr(out), _ptr(pt), _ptr(ev),
                                     _ptr(st.t), _stream())
        self._finish(rc, "capamd_duet_forward", st, check)
        res = (out,) + ((pt,) if parts else ()) + ((ev[:, :, 0], ev[:, :, 1:]) if evidence else ())
        return res if len(res) > 1 else out


QUERY_SIDE, DOC_SIDE = 0, 1        # the `side` of the tower entries: which id-range bit a bad id sets


def cos_sigmoid_pairs(qrep, drep, pair_q=None, pair_d=None, check=True):
    """fp32 tower outputs qrep [Nq, R], drep [Nd, R] (and int32 row indices [n_pairs]; None: pair i is row i) -> fp32 scores
    sigmoid(cos) [n_pairs] through capamd_cos_sigmoid_pairs"""
    _need_gpu(qrep, drep, pair_q, pair_d)
    q, d = _f32(qrep), _f32(drep)
    if q.dim() != 2 or d.dim() != 2 or q.shape[1] != d.shape[1]:
        raise ValueError(f"tower outputs of shapes {tuple(q.shape)} and {tuple(d.shape)}")
    pq, pd = (None if p is None else _i32(p).reshape(-1) for p in (pair_q, pair_d))
    n = pq.numel() if pq is not None else pd.numel() if pd is not None else q.shape[0]
    if (pq is not None and pd is not None and pq.numel() != pd.numel()) or (pq is None and n > q.shape[0]) or (pd is None and n > d.shape[0]):
        raise ValueError(f"{n} pairs for {q.shape[0]} query rows and {d.shape[0]} document rows: without an index array pair i is row i")
    out = torch.empty(n, dtype=torch.float32, device=q.device)
    st = status_word(q.device)
    rc = _lib.load().capamd_cos_sigmoid_pairs(_ptr(q), _ptr(d), _ptr(pq), _ptr(pd), q.shape[0], d.shape[0], n, q.shape[1], _ptr(out), _ptr(st.t), _stream())
    _PerDocumentEngine._finish(rc, "capamd_cos_sigmoid_pairs", st, check)
    return out


class CdssmEngine:
    """CDSSM (reference CDSSM.py, CDSSM_class.forward) through capamd_cdssm_tower, once per side, and capamd_cos_sigmoid_pairs.  The
    embedding table and the convolution are read in place from the live tensors: there is nothing to re-lay out, and no workspace
    beyond the two tower outputs."""

    @staticmethod
    def tower(ids, params, windowsize, side, check=True):
        """int64 ids [N, T] -> fp32 [N, windowsize dim - nkernel + 1], the max over windows and filters, not normalised"""
        _need_gpu(ids)
        x = _i64(ids)
        if x.dim() != 2:
            raise ValueError(f"term ids are [N, T]; got {tuple(x.shape)}")
        emb, w, b = (_f32(params[k].detach()) for k in ("embedding.weight", "conv.0.weight", "conv.0.bias"))
        _need_gpu(emb, w, b)
        N, T = x.shape
        V, D = emb.shape
        F, nk, W = w.shape[0], w.shape[2], int(windowsize)
        if not (1 <= D <= 512 and 1 <= W <= 8 and W * D <= 4096 and 1 <= nk <= min(16, W * D) and 1 <= F <= 16 and T >= 1):
            raise ValueError(f"unsupported CDSSM geometry: dim {D}, windowsize {W}, nkernel {nk}, nfilter {F}, T {T} (dim <= 512, windowsize <= 8, "
                             f"windowsize dim <= 4096, nkernel <= min(16, windowsize dim), nfilter <= 16, T >= 1)")
        rep = torch.empty((N, W * D - nk + 1), dtype=torch.float32, device=x.device)
        st = status_word(x.device)
        rc = _lib.load().capamd_cdssm_tower(_ptr(x), N, T, _ptr(emb), V, D, W, _ptr(w), _ptr(b), nk, F, side, _ptr(rep), _ptr(st.t), _stream())
        _PerDocumentEngine._finish(rc, "capamd_cdssm_tower", st, check)
        return rep

    def forward(self, query, doc, params, windowsize, pair_q=None, pair_d=None, towers=False, check=True):
        """int64 query ids [Nq, Q], document ids [Nd, L] -> fp32 scores (pair i = row i of both, or the int32 index arrays' pairs); with
        towers=True also the two tower outputs"""
        if pair_q is None and pair_d is None and query.shape[0] != doc.shape[0]:
            raise ValueError(f"{query.shape[0]} query rows for {doc.shape[0]} documents")
        qrep = self.tower(query, params, windowsize, QUERY_SIDE, check)
        drep = self.tower(doc, params, windowsize, DOC_SIDE, check)
        out = cos_sigmoid_pairs(qrep, drep, pair_q, pair_d, check)
        return (out, qrep, drep) if towers else out


class DssmEngine:
    """DSSM (reference DSSM.py, DSSM_class.forward) through capamd_dssm_tower, once per side, and capamd_cos_sigmoid_pairs.  The first
    layer is transposed and its rows padded to a multiple of 64 floats once per set of weights, kept until that parameter changes
    (storage pointer + version counter, as TKEngine); the other layers are read in place.  No workspace beyond the two tower outputs."""

    def __init__(self):
        self._key = None
        self._w1t = None

    def model(self, linears):
        """the capamd_dssm_model of the live (weight, bias) pairs of ffw.linear0 ..; the second item keeps what it points to alive"""
        if not 1 <= len(linears) <= 4:
            raise ValueError(f"DSSM takes 1 to 4 layers; got {len(linears)}")
        keep = [(_f32(w.detach()), _f32(b.detach())) for w, b in linears]
        _need_gpu(*(t for wb in keep for t in wb))
        w1 = linears[0][0]
        key = (w1.data_ptr(), w1._version, tuple(w1.shape))
        if key != self._key:
            h1, nvocab = w1.shape
            w1t = torch.zeros((nvocab, _up64(h1)), dtype=torch.float32, device=w1.device)
            w1t[:, :h1] = keep[0][0].t()
            self._w1t, self._key = w1t, key
        m = _lib.DssmModel()
        m.w1t, m.b1 = self._w1t.data_ptr(), keep[0][1].data_ptr()
        m.nvocab, m.layers = self._w1t.shape[0], len(keep)
        for l, (w, b) in enumerate(keep):
            m.width[l] = w.shape[0]
            if l:
                m.w[l - 1], m.b[l - 1] = w.data_ptr(), b.data_ptr()
        return m, (keep, self._w1t)

    def tower(self, bags, linears, side, check=True):
        """Bags of N rows -> fp32 [N, last width], the output of the last ReLU, not normalised"""
        indptr, idx, val = _i64(bags.indptr), _i32(bags.idx), _f32(bags.val)
        _need_gpu(indptr, idx, val)
        m, keep = self.model(linears)
        N = indptr.numel() - 1
        if N < 0 or idx.numel() != val.numel():
            raise ValueError(f"bags with indptr of {indptr.numel()} entries, {idx.numel()} indices and {val.numel()} values")
        rep = torch.empty((N, m.width[m.layers - 1]), dtype=torch.float32, device=indptr.device)
        st = status_word(indptr.device)
        rc = _lib.load().capamd_dssm_tower(_ptr(indptr), _ptr(idx), _ptr(val), N, idx.numel(), ctypes.byref(m), side, _ptr(rep), _ptr(st.t), _stream())
        _PerDocumentEngine._finish(rc, "capamd_dssm_tower", st, check)
        return rep

    def forward(self, query, doc, linears, pair_q=None, pair_d=None, towers=False, check=True):
        """query Bags, document Bags -> fp32 scores (pair i = row i of both, or the int32 index arrays' pairs); with towers=True also
        the two tower outputs"""
        if pair_q is None and pair_d is None and query.rows != doc.rows:
            raise ValueError(f"{query.rows} query bags for {doc.rows} document bags")
        qrep = self.tower(query, linears, QUERY_SIDE, check)
        drep = self.tower(doc, linears, DOC_SIDE, check)
        out = cos_sigmoid_pairs(qrep, drep, pair_q, pair_d, check)
        return (out, qrep, drep) if towers else out
